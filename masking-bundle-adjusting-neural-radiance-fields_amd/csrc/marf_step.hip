// marf_step.hip -- the fused training step of the planar render loop on gfx950.
//
// One block = one tile of TP pixel slots of the crop grid.  Because the target and the mask are
// known when Graph.forward runs (model/planar.py:329-336 -> compute_loss :355-391), the tile's whole
// forward AND backward run in one pass, activations resident in one LDS tile:
//
//   grid -> sl(3) warp -> posenc + c2f                 (warp.py:33-81, model/planar.py:451-471)
//   (Linear + ReLU) x (n-1) -> Linear -> sigmoid       (model/planar.py:429-449)      -> rgb
//   masked MSE: loss partial, d rgb = 2 (p - g) m m    (model/planar.py:382-391), unit upstream
//                                                       gradient and no 1/denominator: both
//                                                       multiply every gradient and are applied
//                                                       in the reduction kernels (gout / denom)
//   sigmoid' -> last-layer weight gradient (16x16 MFMA over the tile's pixels, feat_{n-1} is
//   still in LDS) -> dgrad chain W_l^T with the ReLU masks -> dz_l saved for the hidden-layer
//   weight gradients -> layer-0 dgrad -> posenc / warp adjoint -> dH[3x3] partial per tile.
//
// HBM traffic per pixel (bf16, C3: L=16, 4 x 256 hidden): writes feat_0..feat_{n-2} and
// dz_1..dz_{n-1} (192 + 3*512 + 4*512 B), the ReLU masks (4 * 32 B, read back by the same wave)
// and rgb (12 B); reads target + mask (16 B).  Against the separate forward / loss / backward
// kernels this drops the last layer's input (written and read back, 1 KB), rgb / d rgb round
// trips and a second prologue.
//
// The kernel works on a TileView<P> (marf_gemm.h: a phase is written once over a tile view, a recipe
// is a view).  The epilogues and the loss tail (step_target, step_loss_slots, step_tile_partials,
// step_wlast_grad, step_fill_d) are the functions k_mlp_step_split runs over its split view; only the
// last layer's MFMA loop is written out here, for its prefetched weight fragments.
#include "marf_gemm.h"

namespace marf {

#define STAMP(i) MARF_STAMP(sp, i)

// BL: every forward bias staged in LDS at the start (sum of the hidden widths <= MARF_STEP_NBIAS):
// a GEMM's accumulator init reads LDS instead of loading from global behind the previous GEMM's
// stores (vmcnt retires in issue order), and no bias registers are live across the prologue.
constexpr int MARF_STEP_NBIAS = 1024;

// NW = waves per block: 4 (two blocks per CU) or 8 (one 512-thread block per CU, two waves per
// SIMD: the 512-wide C5 net at TP = 128, where every weight fragment a wave loads from L2 feeds 4
// pixel tiles' MFMAs instead of 2 -- half the weight-fragment traffic per MFMA of TP = 64)
// SK: the net has skip layers (their prologue / posenc-gradient code is compiled in only then: it
// costs the plain nets registers and spills)
// WO: warp-only (a frozen image, marf_warp_step_forward): no tile is queued for saving (the view's
// store stays cleared, so no GEMM flushes one), no last-layer weight / bias gradient partials; the
// ReLU records stay (this kernel's own dgrad re-reads them)
template <class P, int TP, bool BL, int NW, bool SK, bool WO = false>
__global__ __launch_bounds__(64 * NW, NW == 4 ? 2 : 1) void k_mlp_step(StepArgs a) {
    typedef typename P::T T;
    constexpr int PT = TP / 32;
    constexpr int RT = 8 / PT;
    static_assert(TP % (16 * NW) == 0, "last layer: whole 16-pixel groups per wave");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float wsh[32];
    __shared__ float red[(NW * 64 > 2 * TP ? NW * 64 : 2 * TP) * 2];
    __shared__ float red9[NW * 9];
    __shared__ __attribute__((aligned(16))) float gl[TP][4];  // sigmoid' gradient per slot (fp32)
    __shared__ __attribute__((aligned(16))) T gT[8][TP];      // the same, channel-major, split hi / lo
    __shared__ float lsum[2][TP];                              // per-slot ((p-g) m)^2 and m
    __shared__ __attribute__((aligned(16))) float bsh[BL ? MARF_STEP_NBIAS : 4];  // forward biases

    const NetDev& net = a.net;
    TileView<P> v(smem, a.lda, TP);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int b, p0;
    long long slot0;
    tile_origin(a.geo, blockIdx.x, TP, b, p0, slot0);
    const int nl = net.n_layers;
#ifdef MARF_STAMPS
    unsigned long long* sp = a.stamps ? a.stamps + (size_t)blockIdx.x * 32 : nullptr;
#endif

    STAMP(0);
    // the band weights first: vmcnt retires loads in issue order, so the barrier below must not
    // wait behind the tile's HBM target loads (those stay in flight through the prologue)
    const float cw = (int)threadIdx.x < net.L ? a.c2f_w[threadIdx.x] : 0.f;
    if constexpr (BL) {
        for (int l = 0, off = 0; l < nl - 1; off += net.Mp[l], ++l)
            for (int e = threadIdx.x; e < net.Mp[l]; e += 64 * NW) bsh[off + e] = net.bias[l][e];
    }
    // target + mask of the tile's slots: loaded now, parked in gl until the loss needs them; the
    // barrier below waits for the band weights only (step_target)
    const float4 tg = step_target<TP>(a, b, p0);
    if ((int)threadIdx.x < net.L) wsh[threadIdx.x] = cw;
    __syncthreads();
    STAMP(19);
    tile_prologue<P, TP, true, NW>(net, a.geo, a.c2f.on, wsh, v.act, v.lda, b, p0);
    if ((int)threadIdx.x < TP) st_as<float4>(&gl[threadIdx.x][0], tg);
    __syncthreads();
    STAMP(1);
    // every saved tile streams out during the GEMM that reads it next (TileStore)
    if constexpr (!WO) v.template queue_save<NW>(a.feat[0], slot0, 0, TP, net.Kp[0], MARF_DIAG_SAVE(net));

    // ---- hidden layers (forward); the last one is peeled so the last layer's weight fragments
    //      can be in flight behind its epilogue without pinning registers through the loop
    int boff = 0;  // offset of layer l's bias in bsh
    auto bias_of = [&](int l) -> const float* {
        if constexpr (BL) return bsh + boff;
        else return net.bias[l];
    };
    auto hidden = [&](int l) {
        const int K = net.Kp[l], M = net.Mp[l];
        f32x16 acc[RT][PT];
        v.template gemm<RT, PT, NW>(acc, net.Wf[l], M, K, bias_of(l), wave, lane);
        boff += M;
        __syncthreads();  // every wave has consumed the layer input
        STAMP(2 + 2 * l);
        relu_epilogue<RT, PT, NW>(acc, v, M / 32, wave, lane, a.mask_bits[l + 1], blockIdx.x, net.diag[l + 1]);
        __syncthreads();
        if (l < 3) STAMP(3 + 2 * l);
        if (SK && ((net.skip >> (l + 1)) & 1u)) {  // skip layer: [feature ; posenc] (model/planar.py:440-441)
            tile_prologue<P, TP, true, NW>(net, a.geo, a.c2f.on, wsh, v.act, v.lda, b, p0, M);
            __syncthreads();
        }
        v.clear_save();
        if (!WO && l + 1 < nl - 1) {  // the last layer's input never leaves LDS
            const int Kn = net.Kp[l + 1];  // (M + Kp0 for a skip layer)
            v.template queue_save<NW>(a.feat[l + 1], slot0, 0, TP, Kn, MARF_DIAG_SAVE(net));
        }
    };
    for (int l = 0; l < nl - 2; ++l) hidden(l);
    constexpr int NWL = 8;  // prefetched last-layer k-steps (16x16 fragments)
    typename P::frag wl[NWL];
    const T* Wlast = reinterpret_cast<const T*>(net.Wf[nl - 1]);
    const int Kl = net.Kp[nl - 1];
    const int nk16 = Kl / P::KS16;
    {
        const int l = nl - 2;
        const int K = net.Kp[l], M = net.Mp[l];
        f32x16 acc[RT][PT];
        v.template gemm<RT, PT, NW>(acc, net.Wf[l], M, K, bias_of(l), wave, lane);
        __syncthreads();
        STAMP(2 + 2 * l);
#pragma unroll
        for (int u = 0; u < NWL; ++u) wl[u] = P::load_frag(Wlast + ((size_t)(u < nk16 ? u : 0) * 64 + lane) * P::FE);
        relu_epilogue<RT, PT, NW>(acc, v, M / 32, wave, lane, a.mask_bits[l + 1], blockIdx.x, net.diag[l + 1]);
        __syncthreads();
        v.clear_save();
    }

    // ---- last layer (3 outputs, rows padded to 16): mirrors last_layer_gemm (marf_gemm.h), written
    //      out with the first NWL weight fragments prefetched above -- this kernel's scheduling alone;
    //      through the view's w16 / mma16_row the 64-slot instantiations spilled one register more --
    //      then sigmoid, rgb, masked-MSE partial and d rgb, sigmoid backward -> gl (step_loss_slots)
    {
        constexpr int NJ = TP / NW / 16;
        f32x4 acc[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[j] = (f32x4){};
#pragma unroll
        for (int u = 0; u < NWL; ++u) {
            if (u < nk16) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const int px = wave * (TP / NW) + j * 16 + (lane & 15);
                    typename P::frag bb = P::load_frag(v.act + (size_t)px * v.lda + u * P::KS16 + P::kofs16(lane));
                    acc[j] = P::mma16(wl[u], bb, acc[j]);
                }
            }
        }
        for (int u = NWL; u < nk16; ++u) {
            typename P::frag wa = P::load_frag(Wlast + ((size_t)u * 64 + lane) * P::FE);
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int px = wave * (TP / NW) + j * 16 + (lane & 15);
                typename P::frag bb = P::load_frag(v.act + (size_t)px * v.lda + u * P::KS16 + P::kofs16(lane));
                acc[j] = P::mma16(wa, bb, acc[j]);
            }
        }
        step_loss_slots<P, TP, NW>(a, acc, wave, lane, b, p0, gl, gT, lsum);
    }
    __syncthreads();

    STAMP(9);
    step_tile_partials<TP, !WO>(a, wave, lane, gl, lsum);
    if constexpr (!WO) step_wlast_grad<P, TP, NW>(a, Kl, v.feat(), v.lda, wave, lane, gT);
    __syncthreads();  // feat_{n-1} consumed

    step_fill_d<TP>(v, gl, net.Mt[nl - 1], net.diag[nl - 1]);
    STAMP(10);
    __syncthreads();

    // ---- dgrad chain, l = n-1 .. 1 : dfeat_l = W_l^T dz_{l+1}; dz_l = dfeat_l * relu'(feat_l)
    v.clear_save();
    float* dsk = nullptr;  // skip nets: the posenc gradient of the skip layers
    if (SK && net.skip) {
        dsk = reinterpret_cast<float*>(smem + skip_lds_off<P, TP>(net, v.lda));
        for (int e = threadIdx.x; e < TP * net.Kp[0]; e += 64 * NW) dsk[e] = 0.f;
    }
    for (int l = nl - 1; l >= 1; --l) {
        const int R = net.Kp[l], Kk = net.Mt[l];
        f32x16 acc[RT][PT];
        const uint4 mw = *mask_record(a.mask_bits[l], blockIdx.x, wave, lane, NW);  // in flight behind the GEMM
        v.template gemm<RT, PT, NW>(acc, net.Wt[l], R, Kk, nullptr, wave, lane);
        __syncthreads();
        dgrad_epilogue<RT, PT, NW>(acc, net, l, v, wave, lane, mw, dsk);
        __syncthreads();
        if (l <= 4) STAMP(15 - l);  // 14 .. 11
        if constexpr (!WO) v.template queue_save<NW>(a.dz[l], slot0, 0, TP, R, MARF_DIAG_SAVE(net));
    }

    // ---- layer-0 dgrad + posenc / warp adjoint -> dH partial
#ifdef MARF_STAMPS
    warp_adjoint<P, TP, true, NW>(net, a.geo, a.c2f.on, wsh, smem, v.lda, wave, lane, b, p0, red, red9, a.dH_partial, nullptr, v.st,
                                  sp, dsk);
#else
    warp_adjoint<P, TP, true, NW>(net, a.geo, a.c2f.on, wsh, smem, v.lda, wave, lane, b, p0, red, red9, a.dH_partial, nullptr, v.st,
                                  nullptr, dsk);
#endif
    STAMP(15);
}

// The step's c2f band weights, once (model/planar.py:462-470; 1 without c2f).
// (+ an optional int copy riding along: the step kernel's layer-0 column map, one launch fewer)
__global__ void k_c2f_weights(C2fDev c, int L, float* __restrict__ out, const int* __restrict__ csrc,
                              int* __restrict__ cdst, int cn) {
    if ((int)threadIdx.x < L) out[threadIdx.x] = c.on ? c2f_weight(*c.progress, c.start, c.span, L, threadIdx.x) : 1.0f;
    for (int i = threadIdx.x; i < cn; i += blockDim.x) cdst[i] = csrc[i];
}

// Loss of the fused step from the per-tile partials (fp64, fixed-order tree):
// out[0] = f32(sum x^2) / denom, out[1] = denom (= denom_override or 3 * f32(sum m)),
// out[2] = local 3 * f32(sum m)  (model/planar.py:390, as k_mse_final).
__global__ __launch_bounds__(256) void k_loss_final(const double* __restrict__ part, int n, float* __restrict__ out,
                                                    const float* __restrict__ denom_override) {
    __shared__ double rn[256], rm[256];
    double num = 0.0, ms = 0.0;
    // unrolled so 8 partial loads are in flight per thread (latency-bound single block); the
    // per-thread summation order is unchanged
#pragma unroll 8
    for (int i = threadIdx.x; i < n; i += 256) {
        num += part[2 * (size_t)i];
        ms += part[2 * (size_t)i + 1];
    }
    rn[threadIdx.x] = num;
    rm[threadIdx.x] = ms;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            rn[threadIdx.x] += rn[threadIdx.x + o];
            rm[threadIdx.x] += rm[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float denom = denom_override ? denom_override[0] : (float)rm[0] * 3.0f;
        out[0] = (float)rn[0] / denom;
        out[1] = denom;
        out[2] = (float)rm[0] * 3.0f;
    }
}

}  // namespace marf

using namespace marf;

template <class P, int TP, bool BL, int NW, bool SK, bool WO>
static hipError_t launch_step_sk(const StepArgs& a, size_t lds, int n_tiles, hipStream_t s) {
    {
        hipError_t e = ensure_dynamic_lds((const void*)k_mlp_step<P, TP, BL, NW, SK, WO>, lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_mlp_step<P, TP, BL, NW, SK, WO>), dim3(n_tiles), dim3(64 * NW), lds, s, a);
    return hipGetLastError();
}

template <class P, int TP, bool BL, int NW, bool WO>
static hipError_t launch_step_t(const StepArgs& a, size_t lds, int n_tiles, hipStream_t s) {
    return a.net.skip ? launch_step_sk<P, TP, BL, NW, true, WO>(a, lds, n_tiles, s)
                      : launch_step_sk<P, TP, BL, NW, false, WO>(a, lds, n_tiles, s);
}

template <class P, int TP, int NW, bool WO>
static hipError_t launch_step_b(const StepArgs& a, size_t lds, int n_tiles, hipStream_t s) {
    int nb = 0;
    for (int l = 0; l + 1 < a.net.n_layers; ++l) nb += a.net.Mp[l];
    if (nb <= MARF_STEP_NBIAS) return launch_step_t<P, TP, true, NW, WO>(a, lds, n_tiles, s);
    return launch_step_t<P, TP, false, NW, WO>(a, lds, n_tiles, s);
}

template <class P, bool WO>
static hipError_t launch_step_p(const StepArgs& a, int TP, int NW, size_t lds, int n_tiles, hipStream_t s) {
    if (TP == 128 && NW == 8) return launch_step_b<P, 128, 8, WO>(a, lds, n_tiles, s);
    if (NW != 4) return hipErrorInvalidValue;
    return TP == 128 ? launch_step_b<P, 128, 4, WO>(a, lds, n_tiles, s) : launch_step_b<P, 64, 4, WO>(a, lds, n_tiles, s);
}

template <bool WO>
static hipError_t launch_step_d(const StepArgs& a, int dtype, int TP, int NW, size_t lds, int n_tiles, hipStream_t s) {
    if (dtype == 1) return launch_step_p<PrecBF16, WO>(a, TP, NW, lds, n_tiles, s);
    if (dtype == 2) return launch_step_p<PrecF16, WO>(a, TP, NW, lds, n_tiles, s);
    if (NW != 4) return hipErrorInvalidValue;
    return TP == 128 ? launch_step_b<PrecF32, 128, 4, WO>(a, lds, n_tiles, s) : launch_step_b<PrecF32, 64, 4, WO>(a, lds, n_tiles, s);
}

// TP pixel slots per block tile, NW waves per block (4, or 8 for the 16-bit recipes at TP = 128);
// warp_only: k_mlp_step's WO instantiations
hipError_t marf_launch_mlp_step(const StepArgs& a, int dtype, int TP, int NW, size_t lds, int n_tiles, hipStream_t s,
                                bool warp_only) {
    return warp_only ? launch_step_d<true>(a, dtype, TP, NW, lds, n_tiles, s)
                     : launch_step_d<false>(a, dtype, TP, NW, lds, n_tiles, s);
}

hipError_t marf_launch_c2f_weights(const C2fDev& c, int L, float* out, hipStream_t s, const int* csrc, int* cdst,
                                   int cn) {
    hipLaunchKernelGGL(k_c2f_weights, dim3(1), dim3(64), 0, s, c, L, out, csrc, cdst, cn);
    return hipGetLastError();
}

hipError_t marf_launch_loss_final(const double* part, int n, float* out, const float* denom_override, hipStream_t s) {
    hipLaunchKernelGGL(k_loss_final, dim3(1), dim3(256), 0, s, part, n, out, denom_override);
    return hipGetLastError();
}
