// marf_mask.hip -- the learned implicit mask (reference model/planar.py:319-327, 340-352, 475-518):
//
//   k_mask_fwd : per tile of 64 pixel slots, the layer-0 input [E[r] ; E[g] ; E[b] ; uv] built in
//                LDS (embedding_view rows gathered by the pixel's three int32 indices, uv =
//                PosEmbedding(9, 10) of the unwarped crop grid point: [x, y, sin(2^k x), sin(2^k y),
//                cos(2^k x), cos(2^k y), ...], no pi), then Linear+ReLU x (n-1) -> Linear -> sigmoid
//                on the tile kernels' building blocks (marf_gemm.h).  Writes m as [B][1][Np], the
//                layout the fused step reads its mask in; optionally saves every layer input and
//                the ReLU mask records for the backward.
//   k_mask_bwd : per tile, sigmoid' and the dgrad chain through layers n-1 .. 1 with the saved ReLU
//                records, writing dz_l and glast for the generic weight-gradient launchers
//                (marf_wgrad.hip).  Layer 0's dgrad is not run: its input has no trained parameter
//                (embedding_view is in no optimizer group, model/planar.py:93-96).
//   k_mse_mask_bwd : d (gout * rgb_loss) / d m of the masked MSE sum((p - g) m)^2 / (3 sum m)
//                (model/planar.py:388-390) for a soft mask, every scalar read on the device.
//
// 256 threads = 4 waves per block, TP = 64 pixel slots: the 448-wide fp32 input tile is 115 KB,
// inside the 160 KB of a CU.  Each kernel is written once over a tile view (marf_gemm.h) and built for
// two: fp32 (TileView<PrecF32>, exact fp32 MFMA) and the all-operands-split bf16 recipe MARF_BF16X3A
// (SplitView<true>: both planes saved); see the launchers.
#include "marf_gemm.h"

namespace marf {

constexpr int MASK_TP = 64;

// Layer-0 input of the tile's slots into act [TP][lda]; padded columns and padding slots are zero.
template <class V>
MARF_DEV void mask_prologue(const MaskFwdArgs& a, V v, int b, int p0) {
    constexpr int TP = MASK_TP;
    const GeoDev& g = a.geo;
    const int ED = a.embed_dim, NF = a.n_freqs;
    const int q4 = ED / 4;  // float4 groups per embedding row
    // ---- three embedding rows per pixel: column c * ED + j = E[index[b][c][p]][j]
    for (int e = threadIdx.x; e < TP * 3 * q4; e += blockDim.x) {
        const int i = e / (3 * q4), r = e - i * 3 * q4;
        const int c = r / q4, j = (r - c * q4) * 4;
        const int p = p0 + i;
        float4 ev = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p < g.Np) {
            int row = a.index[((size_t)b * 3 + c) * g.Np + p];
            row = row < 0 ? 0 : (row >= a.n_vocab ? a.n_vocab - 1 : row);  // never read outside the table
            ev = ld_as<float4>(a.embed + (size_t)row * ED + j);
        }
        v.put4(v.row(i) + c * ED + j, ev.x, ev.y, ev.z, ev.w);
    }
    // ---- uv: [x, y] then per band k: sin(2^k x), sin(2^k y), cos(2^k x), cos(2^k y)
    const int U0 = 3 * ED;
    for (int e = threadIdx.x; e < TP * 2 * (NF + 1); e += blockDim.x) {
        const int i = e / (2 * (NF + 1)), r = e - i * 2 * (NF + 1);
        const int kk = r >> 1, c = r & 1;  // kk = 0: the raw coordinate; band kk - 1 otherwise
        const int p = p0 + i;
        float x = 0.f;
        const bool valid = p < g.Np;
        if (valid) {
            const int pr = p / g.w, pc = p - pr * g.w;
            x = c ? grid_coord(g.y0 + pr, g.H, g.norm_h) : grid_coord(g.x0 + pc, g.W, g.norm_w);
        }
        if (kk == 0) {
            v.put(v.row(i) + U0 + c, x);
        } else {
            float sv = 0.f, cv = 0.f;
            if (valid) sincosf(ldexpf(x, kk - 1), &sv, &cv);
            v.put(v.row(i) + U0 + 2 + 4 * (kk - 1) + c, sv);
            v.put(v.row(i) + U0 + 2 + 4 * (kk - 1) + 2 + c, cv);
        }
    }
    // ---- zero padding D .. Kp0
    const int D = a.net.D, npad = a.net.Kp[0] - D;
    for (int e = threadIdx.x; e < TP * npad; e += blockDim.x) {
        const int i = e / npad, c = e - i * npad;
        v.zero(v.row(i) + D + c);
    }
}

// The two recipes are the two views.  MaskF32: the fp32 tile, two blocks per CU.  MaskSplit
// (MARF_BF16X3A): two bf16 planes [TP][lda], lda = Kmax + 8 (the fp32 tile's bytes), one block per CU
// (the tile is 114 KB), so a wave may take the whole register file.  Its saved tensors: feat_l
// (l < n-1) and dz_l as two [S][Kp_l] bf16 planes, hi then lo (the fp32 path's bytes per pixel, rows
// 16-B aligned); feat_{n-1}, the input of the one-row last layer, as fp32 [S][Kp] (float(hi) +
// float(lo), the same bytes), which the fp32 last-layer weight gradient reads with glast.
typedef TileView<PrecF32> MaskF32;
typedef SplitView<true> MaskSplit;

template <class V>
__global__ __launch_bounds__(256, V::SPLIT ? 1 : 2) void k_mask_fwd(MaskFwdArgs a) {
    constexpr int TP = MASK_TP;
    constexpr int PT = TP / 32;
    constexpr int RT = 8 / PT;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const NetDev& net = a.net;
    V v(smem, a.lda, TP);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int b, p0;
    long long slot0;
    tile_origin(a.geo, blockIdx.x, TP, b, p0, slot0);
    const long long S = (long long)a.geo.B * a.geo.Np_pad;

    mask_prologue(a, v, b, p0);
    __syncthreads();
    if (a.feat[0]) v.template queue_save<4>(a.feat[0], slot0, S, TP, net.Kp[0]);

    // ---- hidden layers
    const int nl = net.n_layers;
    for (int l = 0; l < nl - 1; ++l) {
        const int K = net.Kp[l], M = net.Mp[l];
        f32x16 acc[RT][PT];
        v.template gemm<RT, PT, 4>(acc, net.Wf[l], M, K, net.bias[l], wave, lane);
        __syncthreads();  // every wave has consumed the layer input
        relu_epilogue<RT, PT>(acc, v, M / 32, wave, lane, a.mask[l + 1], blockIdx.x);
        __syncthreads();
        v.clear_save();
        if (a.feat[l + 1]) {
            if (l + 1 < nl - 1)
                v.template queue_save<4>(a.feat[l + 1], slot0, S, TP, M);
            else  // input of the last (16x16) layer, for the last-layer weight gradient
                v.save_last_input(a.feat[l + 1], slot0, TP, M);
        }
    }

    // ---- last layer: one real output row in the 16-row MFMA form, 16 pixels per wave, sigmoid in fp32
    last_layer_fwd<TP, 4, 1>(v, net, wave, lane, b, p0, a.geo.Np, a.m);
}

template <class V>
__global__ __launch_bounds__(256, V::SPLIT ? 1 : 2) void k_mask_bwd(MaskBwdArgs a) {
    constexpr int TP = MASK_TP;
    constexpr int PT = TP / 32;
    constexpr int RT = 8 / PT;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const NetDev& net = a.net;
    V v(smem, a.lda, TP);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int b, p0;
    long long slot0;
    tile_origin(a.geo, blockIdx.x, TP, b, p0, slot0);
    const long long S = (long long)a.geo.B * a.geo.Np_pad;
    const int nl = net.n_layers;

    // ---- sigmoid backward in fp32: g = (dm * (1 - m)) * m (torch sigmoid_backward); padding slots: zero
    if ((int)threadIdx.x < TP) {
        const int i = threadIdx.x, p = p0 + i;
        float g = 0.f;
        if (p < a.geo.Np) {
            const size_t o = (size_t)b * a.geo.Np + p;
            const float y = a.m[o];
            g = (a.dm[o] * (1.0f - y)) * y;
        }
        st_as<float4>(a.glast + (slot0 + i) * 4, make_float4(g, 0.f, 0.f, 0.f));
        const int Kl = net.Mt[nl - 1];
        for (int c = 0; c < Kl; ++c) v.put(v.row(i) + c, c == 0 ? g : 0.f);
    }
    __syncthreads();

    // ---- dgrad chain, l = nl-1 .. 1 : dfeat_l = W_l^T dz_{l+1}; dz_l = dfeat_l * relu'(feat_l)
    for (int l = nl - 1; l >= 1; --l) {
        const int R = net.Kp[l], Kk = net.Mt[l];
        f32x16 acc[RT][PT];
        const uint4 mw = *mask_record(const_cast<uint64_t*>(a.mask[l]), blockIdx.x, wave, lane);
        v.template gemm<RT, PT, 4>(acc, net.Wt[l], R, Kk, nullptr, wave, lane);
        __syncthreads();
        mask_epilogue<RT, PT>(acc, v, R / 32, wave, lane, mw);
        __syncthreads();
        v.template queue_save<4>(a.dz[l], slot0, S, TP, R);
    }
    v.flush();  // dz_1: no GEMM follows (layer 0's dgrad is not needed)
}

// d (gout * loss) / d m_q, loss = N / D, N = sum m^2 e, e_q = sum_c (p - g)^2, D = 3 sum m:
//   (gout / D) * (2 m_q e_q - 3 loss)      stats = [loss, D, .] as the fused step wrote them
__global__ void k_mse_mask_bwd(const float* __restrict__ pred, const float* __restrict__ gt,
                               const float* __restrict__ mask, int B, int Np, const float* __restrict__ stats,
                               const float* __restrict__ gout, float* __restrict__ d_mask) {
    const long long n = (long long)B * Np;
    const float loss3 = 3.0f * stats[0];
    const float gs = gout[0] / stats[1];
    for (long long e = blockIdx.x * 256LL + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const int b = (int)(e / Np), p = (int)(e % Np);
        const float m = mask[e];
        float me = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float d = pred[e * 3 + c] - gt[((size_t)b * 3 + c) * Np + p];
            me += (d * m) * d;
        }
        d_mask[e] = gs * (2.0f * me - loss3);
    }
}

}  // namespace marf

// ------------------------------------------------------------------ host launchers

using namespace marf;

template <class A>
static hipError_t launch_mask(void (*k)(A), const A& a, size_t lds, int n_tiles, hipStream_t s) {
    hipError_t e = ensure_dynamic_lds((const void*)k, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(n_tiles), dim3(256), lds, s, a);
    return hipGetLastError();
}

// Two recipes: fp32, and (a.split) the all-operands-split bf16 view.  Plain bf16 missed the 1e-2
// gradient bound ("Learned implicit masks"), so no single-16-bit instantiation is built.
hipError_t marf_launch_mask_fwd(const MaskFwdArgs& a, size_t lds, int n_tiles, hipStream_t s) {
    return launch_mask(a.split ? k_mask_fwd<MaskSplit> : k_mask_fwd<MaskF32>, a, lds, n_tiles, s);
}

hipError_t marf_launch_mask_bwd(const MaskBwdArgs& a, size_t lds, int n_tiles, hipStream_t s) {
    return launch_mask(a.split ? k_mask_bwd<MaskSplit> : k_mask_bwd<MaskF32>, a, lds, n_tiles, s);
}

hipError_t marf_launch_mse_mask_bwd(const float* pred, const float* gt, const float* mask, int B, int Np,
                                    const float* stats, const float* gout, float* d_mask, hipStream_t s) {
    long long n = (long long)B * Np;
    long long blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_mse_mask_bwd, dim3((unsigned)blocks), dim3(256), 0, s, pred, gt, mask, B, Np, stats, gout, d_mask);
    return hipGetLastError();
}
