// marf_step2_dev.h -- device functions of the pixel-per-wave step kernel (marf_step2.hip) that
// the weight-gradient kernel (marf_wgrad.hip) runs too when it recomputes a saved tensor instead
// of reading it: the same operations on the same operands, so the same bits.
#pragma once
#include <type_traits>
#include <utility>

#include "marf_common.h"

namespace marf {

// compile-time loop: f(std::integral_constant<int, I>) for I = 0 .. N-1
template <int... I, class F>
MARF_DEV void s2_sfor_impl(std::integer_sequence<int, I...>, F&& f) {
    (f(std::integral_constant<int, I>()), ...);
}
template <int N, class F>
MARF_DEV void s2_sfor(F&& f) {
    s2_sfor_impl(std::make_integer_sequence<int, N>(), f);
}

// LDS-DMA, 4 B per lane (256 B per wave instruction)
MARF_DEV void s2_glds4(const void* src, unsigned lds) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(src), "s"(lds)
                 : "memory");
}

// two floats -> packed bf16 pair (v_cvt_pk_bf16_f32, RNE)
MARF_DEV uint32_t s2_pk(float a, float b) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(((f32x2){a, b}), bf16x2));
}
MARF_DEV float s2_lo16(uint32_t w) { return __uint_as_float(w << 16); }
MARF_DEV float s2_hi16(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }

union S2Frag {
    bf16x8 f;
    f16x8 h;  // (the fp16-forward recipe's operands)
    uint4 u;
    uint32_t w[4];
};

// two floats -> packed fp16 pair (v_cvt_pk_f16_f32, RNE)
MARF_DEV uint32_t s2_pkh(float a, float b) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(((f32x2){a, b}), f16x2));
}

// one k-step of a 32-row output tile: acc += A . B (HF: the fp16x2 recipe's fp16 MFMA)
template <bool HF>
MARF_DEV void s2_mfma(f32x16& acc, const uint4& x, const S2Frag& y) {
    if constexpr (HF)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, x), y.h, acc, 0, 0, 0);
    else
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, x), y.f, acc, 0, 0, 0);
}

// dgrad epilogue of accumulator pair Q (registers 2 Q, 2 Q + 1) of a row tile: x = relu'(z) ? acc : 0
// from the ReLU mask word mw of the tile's pair of row tiles (the forward's mask_pair layout: pair Q
// at bit 7 - Q, the odd elements 16 higher, the even row tile of the pair 8 higher; RTO = rt & 1)
template <int RTO, int Q>
MARF_DEV void s2_bmask_pair(uint32_t mw, const f32x16& pa, float& x0, float& x1) {
    constexpr int b0 = 16 * 0 + 8 * (1 - RTO) + 7 - Q, b1 = 16 * 1 + 8 * (1 - RTO) + 7 - Q;
    x0 = __int_as_float(__builtin_amdgcn_sbfe((int)mw, b0, 1) & __float_as_int(pa[2 * Q]));
    x1 = __int_as_float(__builtin_amdgcn_sbfe((int)mw, b1, 1) & __float_as_int(pa[2 * Q + 1]));
}

// An operand fragment (k-step ks of the lane's pixel: columns 16 ks + 4 h + 0..3 in dwords x, y and
// 16 ks + 8 + 4 h + 0..3 in z, w) -> the lane's 16 bytes of the T16 block layout: two
// v_permlane32_swap exchange the lane halves' x, y <-> z, w, so lane (p, h) holds columns
// 16 ks + 8 h + 0..7 contiguously
MARF_DEV uint4 s2_t16_contig(const S2Frag& f) {
    const auto xz = __builtin_amdgcn_permlane32_swap(f.u.x, f.u.z, false, false);
    const auto yw = __builtin_amdgcn_permlane32_swap(f.u.y, f.u.w, false, false);
    return make_uint4(xz[0], yw[0], xz[1], yw[1]);
}

}  // namespace marf
