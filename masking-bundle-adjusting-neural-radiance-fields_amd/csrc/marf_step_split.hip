// marf_step_split.hip -- the fused training step (and its forward-only render) of MARF_BF16X3 nets
// that the pixel-per-wave kernel k_step2 cannot hold: more than 5 layers, or hidden widths above 256
// (up to 512).  k_mlp_step's phases (marf_step.hip) over the split tile view of marf_gemm.h
// (SplitView<false>; a phase is written once over a view, a recipe is a view -- the epilogues, the
// last layer and the loss tail here are the functions k_mlp_step runs, only the prologue is this
// unit's own): the LDS tile is two bf16 planes [TP][lda] (hi, then lo), every weight image is hi
// then lo, and every GEMM is W_h a_h + W_h a_l + W_l a_h into one fp32 accumulator:
//
//   forward   z = W_h a_h + W_h a_l + W_l a_h (+ bias as the accumulators' start); a' = relu(z) split;
//             layer-0 input = the fp32 prologue's features (exact sincosf), split; the last layer's
//             three rows in the same three terms; sigmoid, masked-MSE partial, d rgb in fp32
//   dgrad     da = W_h^T dz_h + W_h^T dz_l + W_l^T dz_h; dz = da * relu', split in LDS; the layer-0
//             adjoint (posenc, warp, dH partial) in fp32 on the fp32 accumulators
//   saved     the hi planes only: feat_l = a_h and dz_l = (dz)_h as bf16 rows [S][Kp_l], and the ReLU
//             records -- plain bf16's bytes per pixel; the bf16 weight-gradient launchers read them
//
// One 4-wave block per CU (the tile takes 133 - 135 KB of LDS), so a wave may use all 512 registers:
//   hidden width > 256 : TP = 64,  4 row tiles x 2 pixel tiles per wave  (two planes [64][520])
//   hidden width <= 256: TP = 128, 2 row tiles x 4 pixel tiles per wave  (two planes [128][264]): every
//                        weight fragment feeds 4 pixel tiles' MFMAs, and the ReLU records keep plain
//                        bf16's size (one per wave per 128 slots)
// A saved tile's stores go out after the GEMM that reads the tile (gemm_tile_split flushes them).
#include "marf_gemm.h"

namespace marf {

// Prologue with the layer-0 input split: grid -> warp -> posenc (+ c2f) in fp32 as the fp32 tile
// kernel computes them (tile_prologue<PrecF32>: exact sincosf, the band weight multiplied in), each
// feature stored as its bf16 hi and lo.  256 / TP threads share a pixel, the bands dealt round-robin.
template <int TP, bool GRID_ONLY>
MARF_DEV void tile_prologue_split(const NetDev& net, const GeoDev& geo, int c2f_on, const float* wsh, u16* ah, u16* al,
                                  int lda, int b, int p0) {
    constexpr int NPART = 256 / TP;
    const int L = net.L;
    const int i = threadIdx.x % TP, part = threadIdx.x / TP;
    float x, y, u = 0.f, v = 0.f, X[3];
    slot_point<GRID_ONLY>(geo, b, p0 + i, x, y, u, v, X);
    const size_t at = (size_t)i * lda;
    auto put = [&](int col, float f) { split1(f, ah[at + col], al[at + col]); };
    if (part == 0) {
        put(0, u);
        put(1, v);
    }
    for (int q = part; q < 2 * L; q += NPART) {
        const int c = q >= L, k = q - c * L;
        float s, co;
        band_sincos<false>(c ? v : u, k, s, co);
        if (c2f_on) {
            const float w = wsh[k];
            s = s * w;
            co = co * w;
        }
        put(2 + 2 * c * L + k, s);
        put(2 + 2 * c * L + L + k, co);
    }
    for (int f = net.D + part; f < net.Kp[0]; f += NPART) {
        ah[at + f] = 0;
        al[at + f] = 0;
    }
}

// FWD: the render (marf_render): forward only, any geometry, rgb out, nothing saved; the training
// forward's instructions on the same pixels, so the same bits.
// WO: warp-only (a frozen image, marf_warp_step_forward): the training step with no tile queued for
// saving and no last-layer weight / bias gradient partials; the ReLU records stay (the dgrad re-reads
// them).
template <int TP, bool FWD, bool WO = false>
__global__ __launch_bounds__(256, 1) void k_mlp_step_split(StepArgs a) {
    typedef PrecBF16 P;
    constexpr int NW = 4;
    constexpr int PT = TP / 32;
    constexpr int RT = 8 / PT;
    constexpr int NJ = TP / NW / 16;
    constexpr int TS = FWD ? 1 : TP;  // the training-only arrays
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float wsh[32];
    __shared__ float red[FWD ? 1 : (NW * 64 > 2 * TP ? NW * 64 : 2 * TP) * 2];
    __shared__ float red9[NW * 9];
    __shared__ __attribute__((aligned(16))) float gl[TS][4];  // sigmoid' gradient per slot (fp32)
    __shared__ __attribute__((aligned(16))) u16 gT[8][TS];    // the same, channel-major, split hi / lo
    __shared__ float lsum[2][TS];                              // per-slot ((p-g) m)^2 and m

    const NetDev& net = a.net;
    SplitView<false> v(smem, a.lda, TP);  // saved tiles: the hi plane only
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int b, p0;
    long long slot0;
    tile_origin(a.geo, blockIdx.x, TP, b, p0, slot0);
    const int nl = net.n_layers;

    // target + mask of the tile's slots: loaded now, parked in gl until the loss needs them
    float4 tg = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (FWD) {
        c2f_weights_lds(a.c2f, net.L, wsh);
    } else {
        if ((int)threadIdx.x < net.L) wsh[threadIdx.x] = a.c2f_w[threadIdx.x];
        tg = step_target<TP>(a, b, p0);
    }
    __syncthreads();
    tile_prologue_split<TP, !FWD>(net, a.geo, a.c2f.on, wsh, v.hi, v.lo, v.lda, b, p0);
    if constexpr (!FWD) {
        if ((int)threadIdx.x < TP) st_as<float4>(&gl[threadIdx.x][0], tg);
    }
    __syncthreads();

    // the saved tiles stream out after the GEMM that reads the tile
    auto save = [&](void* dst, int cols) {
        if constexpr (!FWD && !WO) v.template queue_save<NW>(dst, slot0, 0, TP, cols);
    };
    save(a.feat[0], net.Kp[0]);

    // ---- hidden layers (forward)
    for (int l = 0; l < nl - 1; ++l) {
        const int K = net.Kp[l], M = net.Mp[l];
        f32x16 acc[RT][PT];
        v.template gemm<RT, PT, NW>(acc, net.Wf[l], M, K, net.bias[l], wave, lane);
        __syncthreads();  // every wave has consumed the layer input
        relu_epilogue<RT, PT, NW>(acc, v, M / 32, wave, lane, FWD ? nullptr : a.mask_bits[l + 1], blockIdx.x);
        __syncthreads();
        v.clear_save();
        if (l + 1 < nl - 1) save(a.feat[l + 1], M);  // the last layer's input never leaves LDS
    }

    // ---- last layer (3 outputs, rows padded to 16): 16x16 MFMA in the same three terms, TP/NW pixels
    //      per wave, then sigmoid (render: to rgb) and the loss tail shared with k_mlp_step, in fp32
    const int Kl = net.Kp[nl - 1];
    if constexpr (FWD) {
        last_layer_fwd<TP, NW, 3>(v, net, wave, lane, b, p0, a.geo.Np, a.rgb);
    } else {
        {
            f32x4 acc[NJ];
            last_layer_gemm<TP, NW>(v, net.Wf[nl - 1], Kl, wave, lane, acc);
            step_loss_slots<P, TP, NW>(a, acc, wave, lane, b, p0, gl, gT, lsum);
        }
        __syncthreads();
        step_tile_partials<TP, !WO>(a, wave, lane, gl, lsum);
        if constexpr (!WO) step_wlast_grad<P, TP, NW>(a, Kl, v.feat(), v.lda, wave, lane, gT);  // B = the hi plane
        __syncthreads();  // feat_{n-1} consumed
        step_fill_d<TP>(v, gl, net.Mt[nl - 1], 0);
        __syncthreads();

        // ---- dgrad chain, l = n-1 .. 1 : da = W_h^T dz_h + W_h^T dz_l + W_l^T dz_h; dz_l = da * relu'
        v.clear_save();
        for (int l = nl - 1; l >= 1; --l) {
            const int R = net.Kp[l], Kk = net.Mt[l];
            f32x16 acc[RT][PT];
            const uint4 mw = *mask_record(a.mask_bits[l], blockIdx.x, wave, lane, NW);  // in flight behind the GEMM
            v.template gemm<RT, PT, NW>(acc, net.Wt[l], R, Kk, nullptr, wave, lane);
            __syncthreads();
            mask_epilogue<RT, PT, NW>(acc, v, R / 32, wave, lane, mw);
            __syncthreads();
            save(a.dz[l], R);
        }

        // ---- layer-0 dgrad (three terms; dz_1's stores go out behind it) + posenc / warp adjoint in
        //      fp32 -> dH partial
        f32x16 acc[RT][PT];
        v.template gemm<RT, PT, NW>(acc, net.Wt[0], net.Kp[0], net.Mt[0], nullptr, wave, lane);
        __syncthreads();
        warp_adjoint_tail<P, TP, true, NW, false>(acc, net, a.geo, a.c2f.on, wsh, smem, wave, lane, b, p0, red, red9,
                                                  a.dH_partial, nullptr, nullptr, nullptr);
    }
}

}  // namespace marf

using namespace marf;

template <int TP, bool FWD, bool WO = false>
static hipError_t launch_split(const StepArgs& a, size_t lds, int n_tiles, hipStream_t s) {
    hipError_t e = ensure_dynamic_lds((const void*)k_mlp_step_split<TP, FWD, WO>, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_mlp_step_split<TP, FWD, WO>), dim3(n_tiles), dim3(256), lds, s, a);
    return hipGetLastError();
}

// TP: 64 (hidden widths above 256) or 128; fwd_only: the render instantiation; warp_only: the WO one
hipError_t marf_launch_mlp_step_split(const StepArgs& a, int TP, bool fwd_only, size_t lds, int n_tiles, hipStream_t s,
                                      bool warp_only) {
    if (warp_only && !fwd_only) {
        if (TP == 64) return launch_split<64, false, true>(a, lds, n_tiles, s);
        if (TP == 128) return launch_split<128, false, true>(a, lds, n_tiles, s);
        return hipErrorInvalidValue;
    }
    if (TP == 64) return fwd_only ? launch_split<64, true>(a, lds, n_tiles, s) : launch_split<64, false>(a, lds, n_tiles, s);
    if (TP == 128) return fwd_only ? launch_split<128, true>(a, lds, n_tiles, s) : launch_split<128, false>(a, lds, n_tiles, s);
    return hipErrorInvalidValue;
}
