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
// inside the 160 KB of a CU.  Built in fp32 (exact fp32 MFMA) and in the all-operands-split bf16 recipe
// MARF_BF16X3A (k_mask_fwd_split / k_mask_bwd_split below; see the launchers).
#include "marf_gemm.h"

namespace marf {

constexpr int MASK_TP = 64;

// Layer-0 input of the tile's slots into act [TP][lda]; padded columns and padding slots are zero.
template <class P>
MARF_DEV void mask_prologue(const MaskFwdArgs& a, typename P::T* act, int lda, int b, int p0) {
    typedef typename P::T T;
    constexpr int TP = MASK_TP;
    const GeoDev& g = a.geo;
    const int ED = a.embed_dim, NF = a.n_freqs;
    const int q4 = ED / 4;  // float4 groups per embedding row
    // ---- three embedding rows per pixel: column c * ED + j = E[index[b][c][p]][j]
    for (int e = threadIdx.x; e < TP * 3 * q4; e += blockDim.x) {
        const int i = e / (3 * q4), r = e - i * 3 * q4;
        const int c = r / q4, j = (r - c * q4) * 4;
        const int p = p0 + i;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p < g.Np) {
            int row = a.index[((size_t)b * 3 + c) * g.Np + p];
            row = row < 0 ? 0 : (row >= a.n_vocab ? a.n_vocab - 1 : row);  // never read outside the table
            v = ld_as<float4>(a.embed + (size_t)row * ED + j);
        }
        store4<P>(act + (size_t)i * lda + c * ED + j, v.x, v.y, v.z, v.w);
    }
    // ---- uv: [x, y] then per band k: sin(2^k x), sin(2^k y), cos(2^k x), cos(2^k y)
    const int U0 = 3 * ED;
    for (int e = threadIdx.x; e < TP * 2 * (NF + 1); e += blockDim.x) {
        const int i = e / (2 * (NF + 1)), r = e - i * 2 * (NF + 1);
        const int kk = r >> 1, c = r & 1;  // kk = 0: the raw coordinate; band kk - 1 otherwise
        const int p = p0 + i;
        T* row = act + (size_t)i * lda + U0;
        float x = 0.f;
        const bool valid = p < g.Np;
        if (valid) {
            const int pr = p / g.w, pc = p - pr * g.w;
            x = c ? grid_coord(g.y0 + pr, g.H, g.norm_h) : grid_coord(g.x0 + pc, g.W, g.norm_w);
        }
        if (kk == 0) {
            row[c] = P::cvt(x);
        } else {
            float sv = 0.f, cv = 0.f;
            if (valid) sincosf(ldexpf(x, kk - 1), &sv, &cv);
            row[2 + 4 * (kk - 1) + c] = P::cvt(sv);
            row[2 + 4 * (kk - 1) + 2 + c] = P::cvt(cv);
        }
    }
    // ---- zero padding D .. Kp0
    const int D = a.net.D, npad = a.net.Kp[0] - D;
    for (int e = threadIdx.x; e < TP * npad; e += blockDim.x) {
        const int i = e / npad, c = e - i * npad;
        act[(size_t)i * lda + D + c] = P::cvt(0.f);
    }
}

template <class P>
__global__ __launch_bounds__(256, 2) void k_mask_fwd(MaskFwdArgs a) {
    typedef typename P::T T;
    constexpr int TP = MASK_TP;
    constexpr int PT = TP / 32;
    constexpr int RT = 8 / PT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* act = reinterpret_cast<T*>(smem);

    const NetDev& net = a.net;
    const int lda = a.lda;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int b, p0;
    long long slot0;
    tile_origin(a.geo, blockIdx.x, TP, b, p0, slot0);

    mask_prologue<P>(a, act, lda, b, p0);
    __syncthreads();
    TileStore<T> st;
    st.clear();
    if (a.feat[0])
        save_tile<P>(st, act, lda, TP, net.Kp[0], reinterpret_cast<T*>(a.feat[0]) + slot0 * net.Kp[0], net.Kp[0] / P::KS);

    // ---- hidden layers
    const int nl = net.n_layers;
    for (int l = 0; l < nl - 1; ++l) {
        const int K = net.Kp[l], M = net.Mp[l], n_rt = M / 32;
        f32x16 acc[RT][PT];
        gemm_tile<P, RT, PT>(acc, reinterpret_cast<const T*>(net.Wf[l]), K, n_rt, act, lda, wave, lane, net.bias[l], st);
        __syncthreads();  // every wave has consumed the layer input
        relu_epilogue<P, RT, PT>(acc, act, lda, n_rt, wave, lane, a.mask[l + 1], blockIdx.x);
        __syncthreads();
        st.clear();
        if (a.feat[l + 1]) {
            if (l + 1 < nl - 1)
                save_tile<P>(st, act, lda, TP, M, reinterpret_cast<T*>(a.feat[l + 1]) + slot0 * M, M / P::KS);
            else  // input of the last (16x16) layer: plain copy
                copy_tile_out<P>(act, lda, TP, M, reinterpret_cast<T*>(a.feat[l + 1]) + slot0 * M, M);
        }
    }

    // ---- last layer: one real output row in the 16-row MFMA form, 16 pixels per wave, sigmoid
    {
        const int l = nl - 1;
        const int K = net.Kp[l];
        const T* W = reinterpret_cast<const T*>(net.Wf[l]);
        f32x4 acc = (f32x4){};
        const int ko = P::kofs16(lane);
        const int px = wave * (TP / 4) + (lane & 15);
        for (int k0 = 0; k0 < K; k0 += P::KS16) {
            typename P::frag wa = P::load_frag(W + ((size_t)(k0 / P::KS16) * 64 + lane) * P::FE);
            typename P::frag bb = P::load_frag(act + (size_t)px * lda + k0 + ko);
            acc = P::mma16(wa, bb, acc);
        }
        if (lane < 16) {
            const int p = p0 + px;
            if (p < a.geo.Np) {
                const float z = acc[0] + net.bias[l][0];
                a.m[(size_t)b * a.geo.Np + p] = 1.0f / (1.0f + expf(-z));
            }
        }
    }
}

template <class P>
__global__ __launch_bounds__(256, 2) void k_mask_bwd(MaskBwdArgs a) {
    typedef typename P::T T;
    constexpr int TP = MASK_TP;
    constexpr int PT = TP / 32;
    constexpr int RT = 8 / PT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* act = reinterpret_cast<T*>(smem);

    const NetDev& net = a.net;
    const int lda = a.lda;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int b, p0;
    long long slot0;
    tile_origin(a.geo, blockIdx.x, TP, b, p0, slot0);
    const int nl = net.n_layers;

    // ---- sigmoid backward: g = (dm * (1 - m)) * m (torch sigmoid_backward); padding slots: zero
    if ((int)threadIdx.x < TP) {
        const int i = threadIdx.x, p = p0 + i;
        float g = 0.f;
        if (p < a.geo.Np) {
            const size_t o = (size_t)b * a.geo.Np + p;
            const float y = a.m[o];
            g = (a.dm[o] * (1.0f - y)) * y;
        }
        st_as<float4>(a.glast + (slot0 + i) * 4, make_float4(g, 0.f, 0.f, 0.f));
        T* row = act + (size_t)i * lda;
        const int Kl = net.Mt[nl - 1];
        for (int c = 0; c < Kl; ++c) row[c] = P::cvt(c == 0 ? g : 0.f);
    }
    __syncthreads();

    // ---- dgrad chain, l = nl-1 .. 1 : dfeat_l = W_l^T dz_{l+1}; dz_l = dfeat_l * relu'(feat_l)
    TileStore<T> st;
    st.clear();
    for (int l = nl - 1; l >= 1; --l) {
        const int R = net.Kp[l], Kk = net.Mt[l], n_rt = R / 32;
        f32x16 acc[RT][PT];
        const uint4 mw = *mask_record(const_cast<uint64_t*>(a.mask[l]), blockIdx.x, wave, lane);
        gemm_tile<P, RT, PT>(acc, reinterpret_cast<const T*>(net.Wt[l]), Kk, n_rt, act, lda, wave, lane, nullptr, st);
        __syncthreads();
        mask_epilogue<P, RT, PT>(acc, act, lda, n_rt, wave, lane, mw);
        __syncthreads();
        save_tile<P>(st, act, lda, TP, R, reinterpret_cast<T*>(a.dz[l]) + slot0 * R, 0);
    }
    if (st.active) st.flush(act);  // dz_1: no GEMM follows (layer 0's dgrad is not needed)
}

// ---- MARF_BF16X3A: every GEMM operand split into bf16 hi + lo (marf_gemm.h, "all-operands-split").
// The LDS tile is two bf16 planes [TP][lda], lda = Kmax + 8 (the fp32 tile's bytes).  Saved tensors:
// feat_l (l < n-1) and dz_l as two [S][Kp_l] bf16 planes, hi then lo (the fp32 path's bytes per
// pixel, rows 16-B aligned); feat_{n-1}, the input of the one-row last layer, as fp32 [S][Kp]
// (float(hi) + float(lo), the same bytes), which the fp32 last-layer weight gradient reads with glast.

// mask_prologue with the layer-0 input split; padded columns and padding slots are zero in both planes.
MARF_DEV void mask_prologue_split(const MaskFwdArgs& a, u16* ah, u16* al, int lda, int b, int p0) {
    constexpr int TP = MASK_TP;
    const GeoDev& g = a.geo;
    const int ED = a.embed_dim, NF = a.n_freqs;
    const int q4 = ED / 4;
    for (int e = threadIdx.x; e < TP * 3 * q4; e += blockDim.x) {
        const int i = e / (3 * q4), r = e - i * 3 * q4;
        const int c = r / q4, j = (r - c * q4) * 4;
        const int p = p0 + i;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p < g.Np) {
            int row = a.index[((size_t)b * 3 + c) * g.Np + p];
            row = row < 0 ? 0 : (row >= a.n_vocab ? a.n_vocab - 1 : row);  // never read outside the table
            v = ld_as<float4>(a.embed + (size_t)row * ED + j);
        }
        const size_t at = (size_t)i * lda + c * ED + j;
        store4_split(ah + at, al + at, v.x, v.y, v.z, v.w);
    }
    const int U0 = 3 * ED;
    for (int e = threadIdx.x; e < TP * 2 * (NF + 1); e += blockDim.x) {
        const int i = e / (2 * (NF + 1)), r = e - i * 2 * (NF + 1);
        const int kk = r >> 1, c = r & 1;
        const int p = p0 + i;
        const size_t at = (size_t)i * lda + U0;
        float x = 0.f;
        const bool valid = p < g.Np;
        if (valid) {
            const int pr = p / g.w, pc = p - pr * g.w;
            x = c ? grid_coord(g.y0 + pr, g.H, g.norm_h) : grid_coord(g.x0 + pc, g.W, g.norm_w);
        }
        if (kk == 0) {
            split1(x, ah[at + c], al[at + c]);
        } else {
            float sv = 0.f, cv = 0.f;
            if (valid) sincosf(ldexpf(x, kk - 1), &sv, &cv);
            const int cs = 2 + 4 * (kk - 1) + c;
            split1(sv, ah[at + cs], al[at + cs]);
            split1(cv, ah[at + cs + 2], al[at + cs + 2]);
        }
    }
    const int D = a.net.D, npad = a.net.Kp[0] - D;
    for (int e = threadIdx.x; e < TP * npad; e += blockDim.x) {
        const int i = e / npad, c = e - i * npad;
        ah[(size_t)i * lda + D + c] = 0;
        al[(size_t)i * lda + D + c] = 0;
    }
}

// One block per CU (the tile is 114 KB), so a wave may take the whole register file.
__global__ __launch_bounds__(256, 1) void k_mask_fwd_split(MaskFwdArgs a) {
    typedef PrecBF16 P;
    constexpr int TP = MASK_TP;
    constexpr int PT = TP / 32;
    constexpr int RT = 8 / PT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const NetDev& net = a.net;
    const int lda = a.lda;
    u16* ah = reinterpret_cast<u16*>(smem);
    u16* al = ah + (size_t)TP * lda;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int b, p0;
    long long slot0;
    tile_origin(a.geo, blockIdx.x, TP, b, p0, slot0);
    const long long S = (long long)a.geo.B * a.geo.Np_pad;

    mask_prologue_split(a, ah, al, lda, b, p0);
    __syncthreads();
    TileStore<u16> sth, stl;
    sth.clear();
    stl.clear();
    auto save_planes = [&](void* dst, int cols) {
        u16* d = reinterpret_cast<u16*>(dst);
        sth.init(lda, d + slot0 * cols, cols, TP, cols, wave, lane);
        stl.init(lda, d + (S + slot0) * cols, cols, TP, cols, wave, lane);
    };
    if (a.feat[0]) save_planes(a.feat[0], net.Kp[0]);

    const int nl = net.n_layers;
    for (int l = 0; l < nl - 1; ++l) {
        const int K = net.Kp[l], M = net.Mp[l];
        f32x16 acc[RT][PT];
        gemm_tile_split<RT, PT>(acc, reinterpret_cast<const u16*>(net.Wf[l]), M, K, ah, al, lda, wave, lane, net.bias[l], sth, stl);
        __syncthreads();  // every wave has consumed the layer input
        relu_epilogue_split<RT, PT>(acc, ah, al, lda, M / 32, wave, lane, a.mask[l + 1], blockIdx.x);
        __syncthreads();
        sth.clear();
        stl.clear();
        if (a.feat[l + 1]) {
            if (l + 1 < nl - 1) {
                save_planes(a.feat[l + 1], M);
            } else {  // input of the last layer: fp32 [S][M] for the fp32 last-layer weight gradient
                float* d = reinterpret_cast<float*>(a.feat[l + 1]) + slot0 * M;
                for (int e = threadIdx.x; e < TP * M; e += blockDim.x) {
                    const int r = e / M, c = e - r * M;
                    d[(size_t)r * M + c] = bf2f(ah[(size_t)r * lda + c]) + bf2f(al[(size_t)r * lda + c]);
                }
            }
        }
    }

    // ---- last layer: one real output row in the 16-row MFMA form, the same three terms, sigmoid in fp32
    {
        const int l = nl - 1;
        const int K = net.Kp[l];
        const u16* Wh = reinterpret_cast<const u16*>(net.Wf[l]);
        const u16* Wl = Wh + (size_t)16 * K;
        f32x4 acc = (f32x4){};
        const int ko = P::kofs16(lane);
        const int px = wave * (TP / 4) + (lane & 15);
        for (int k0 = 0; k0 < K; k0 += P::KS16) {
            const size_t wo = ((size_t)(k0 / P::KS16) * 64 + lane) * P::FE;
            const size_t bo = (size_t)px * lda + k0 + ko;
            const P::frag wh = P::load_frag(Wh + wo), wl = P::load_frag(Wl + wo);
            const P::frag bh = P::load_frag(ah + bo), bl = P::load_frag(al + bo);
            acc = P::mma16(wh, bh, acc);
            acc = P::mma16(wh, bl, acc);
            acc = P::mma16(wl, bh, acc);
        }
        if (lane < 16) {
            const int p = p0 + px;
            if (p < a.geo.Np) {
                const float z = acc[0] + net.bias[l][0];
                a.m[(size_t)b * a.geo.Np + p] = 1.0f / (1.0f + expf(-z));
            }
        }
    }
}

__global__ __launch_bounds__(256, 1) void k_mask_bwd_split(MaskBwdArgs a) {
    constexpr int TP = MASK_TP;
    constexpr int PT = TP / 32;
    constexpr int RT = 8 / PT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const NetDev& net = a.net;
    const int lda = a.lda;
    u16* ah = reinterpret_cast<u16*>(smem);
    u16* al = ah + (size_t)TP * lda;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int b, p0;
    long long slot0;
    tile_origin(a.geo, blockIdx.x, TP, b, p0, slot0);
    const long long S = (long long)a.geo.B * a.geo.Np_pad;
    const int nl = net.n_layers;

    // ---- sigmoid backward in fp32: g = (dm * (1 - m)) * m; padding slots: zero
    if ((int)threadIdx.x < TP) {
        const int i = threadIdx.x, p = p0 + i;
        float g = 0.f;
        if (p < a.geo.Np) {
            const size_t o = (size_t)b * a.geo.Np + p;
            const float y = a.m[o];
            g = (a.dm[o] * (1.0f - y)) * y;
        }
        st_as<float4>(a.glast + (slot0 + i) * 4, make_float4(g, 0.f, 0.f, 0.f));
        u16 gh, gl;
        split1(g, gh, gl);
        const size_t at = (size_t)i * lda;
        const int Kl = net.Mt[nl - 1];
        for (int c = 0; c < Kl; ++c) {
            ah[at + c] = c == 0 ? gh : (u16)0;
            al[at + c] = c == 0 ? gl : (u16)0;
        }
    }
    __syncthreads();

    // ---- dgrad chain, l = nl-1 .. 1 : da = W_h^T dz_h + W_h^T dz_l + W_l^T dz_h; dz_l = da * relu', split
    TileStore<u16> sth, stl;
    sth.clear();
    stl.clear();
    for (int l = nl - 1; l >= 1; --l) {
        const int R = net.Kp[l], Kk = net.Mt[l];
        f32x16 acc[RT][PT];
        const uint4 mw = *mask_record(const_cast<uint64_t*>(a.mask[l]), blockIdx.x, wave, lane);
        gemm_tile_split<RT, PT>(acc, reinterpret_cast<const u16*>(net.Wt[l]), R, Kk, ah, al, lda, wave, lane, nullptr, sth, stl);
        __syncthreads();
        mask_epilogue_split<RT, PT>(acc, ah, al, lda, R / 32, wave, lane, mw);
        __syncthreads();
        u16* d = reinterpret_cast<u16*>(a.dz[l]);
        sth.init(lda, d + slot0 * R, R, TP, R, wave, lane);
        stl.init(lda, d + (S + slot0) * R, R, TP, R, wave, lane);
    }
    if (sth.active) sth.flush(ah);  // dz_1: no GEMM follows (layer 0's dgrad is not needed)
    if (stl.active) stl.flush(al);
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

template <class P>
static hipError_t launch_mask_fwd_t(const MaskFwdArgs& a, size_t lds, int n_tiles, hipStream_t s) {
    hipError_t e = ensure_dynamic_lds((const void*)k_mask_fwd<P>, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_mask_fwd<P>), dim3(n_tiles), dim3(256), lds, s, a);
    return hipGetLastError();
}

template <class P>
static hipError_t launch_mask_bwd_t(const MaskBwdArgs& a, size_t lds, int n_tiles, hipStream_t s) {
    hipError_t e = ensure_dynamic_lds((const void*)k_mask_bwd<P>, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_mask_bwd<P>), dim3(n_tiles), dim3(256), lds, s, a);
    return hipGetLastError();
}

// Two recipes: fp32, and (a.split) the all-operands-split bf16 kernels.  Plain bf16 missed the 1e-2
// gradient bound ("Learned implicit masks"), so no single-16-bit instantiation is built; the
// fp32 kernels stay written against the precision traits.
hipError_t marf_launch_mask_fwd(const MaskFwdArgs& a, size_t lds, int n_tiles, hipStream_t s) {
    if (a.split) {
        hipError_t e = ensure_dynamic_lds((const void*)k_mask_fwd_split, lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_mask_fwd_split, dim3(n_tiles), dim3(256), lds, s, a);
        return hipGetLastError();
    }
    return launch_mask_fwd_t<PrecF32>(a, lds, n_tiles, s);
}

hipError_t marf_launch_mask_bwd(const MaskBwdArgs& a, size_t lds, int n_tiles, hipStream_t s) {
    if (a.split) {
        hipError_t e = ensure_dynamic_lds((const void*)k_mask_bwd_split, lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_mask_bwd_split, dim3(n_tiles), dim3(256), lds, s, a);
        return hipGetLastError();
    }
    return launch_mask_bwd_t<PrecF32>(a, lds, n_tiles, s);
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
