// marf_step_split.hip -- the fused training step (and its forward-only render) of MARF_BF16X3 nets
// that the pixel-per-wave kernel k_step2 cannot hold: more than 5 layers, or hidden widths above 256
// (up to 512).  k_mlp_step's phases (marf_step.hip) on the all-operands-split tile blocks of
// marf_gemm.h: the LDS tile is two bf16 planes [TP][lda] (hi, then lo), every weight image is hi
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
template <int TP, bool FWD>
__global__ __launch_bounds__(256, 1) void k_mlp_step_split(StepArgs a) {
    typedef PrecBF16 P;
    constexpr int NW = 4;
    constexpr int PT = TP / 32;
    constexpr int RT = 8 / PT;
    constexpr int TS = FWD ? 1 : TP;  // the training-only arrays
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float wsh[32];
    __shared__ float red[FWD ? 1 : (NW * 64 > 2 * TP ? NW * 64 : 2 * TP) * 2];
    __shared__ float red9[NW * 9];
    __shared__ __attribute__((aligned(16))) float gl[TS][4];  // sigmoid' gradient per slot (fp32)
    __shared__ __attribute__((aligned(16))) u16 gT[8][TS];    // the same, channel-major, split hi / lo
    __shared__ float lsum[2][TS];                              // per-slot ((p-g) m)^2 and m

    const NetDev& net = a.net;
    const int lda = a.lda;
    u16* ah = reinterpret_cast<u16*>(smem);
    u16* al = ah + (size_t)TP * lda;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int b, p0;
    long long slot0;
    tile_origin(a.geo, blockIdx.x, TP, b, p0, slot0);
    const int nl = net.n_layers;
    const int Np = a.geo.Np;

    // target + mask of the tile's slots: loaded now, parked in gl until the loss needs them
    // (every thread loads, padding slots a clamped valid pixel, zeroed after: as k_mlp_step)
    float4 tg = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (FWD) {
        c2f_weights_lds(a.c2f, net.L, wsh);
    } else {
        if ((int)threadIdx.x < net.L) wsh[threadIdx.x] = a.c2f_w[threadIdx.x];
        const int ti = threadIdx.x & (TP - 1);
        const int pc = min(p0 + ti, Np - 1);
        const float* gb = a.gt + (size_t)b * 3 * Np + pc;
        const float* mb = a.mask ? a.mask + (size_t)b * Np + pc : gb;
        tg = make_float4(gb[0], gb[Np], gb[2 * (size_t)Np], mb[0]);
        if (!a.mask) tg.w = 1.0f;
        if (p0 + ti >= Np) tg = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    tile_prologue_split<TP, !FWD>(net, a.geo, a.c2f.on, wsh, ah, al, lda, b, p0);
    if constexpr (!FWD) {
        if ((int)threadIdx.x < TP) st_as<float4>(&gl[threadIdx.x][0], tg);
    }
    __syncthreads();

    // the saved tiles: hi plane only (stl stays idle), streamed out after the GEMM that reads the tile
    TileStore<u16> sth, stl;
    sth.clear();
    stl.clear();
    auto save_hi = [&](void* dst, int cols) {
        if constexpr (!FWD) sth.init(lda, reinterpret_cast<u16*>(dst) + slot0 * cols, cols, TP, cols, wave, lane, NW);
    };
    save_hi(a.feat[0], net.Kp[0]);

    // ---- hidden layers (forward)
    for (int l = 0; l < nl - 1; ++l) {
        const int K = net.Kp[l], M = net.Mp[l];
        f32x16 acc[RT][PT];
        gemm_tile_split<RT, PT, NW>(acc, reinterpret_cast<const u16*>(net.Wf[l]), M, K, ah, al, lda, wave, lane, net.bias[l],
                                    sth, stl);
        __syncthreads();  // every wave has consumed the layer input
        relu_epilogue_split<RT, PT, NW>(acc, ah, al, lda, M / 32, wave, lane, FWD ? nullptr : a.mask_bits[l + 1], blockIdx.x);
        __syncthreads();
        sth.clear();
        if (l + 1 < nl - 1) save_hi(a.feat[l + 1], M);  // the last layer's input never leaves LDS
    }

    // ---- last layer (3 outputs, rows padded to 16): 16x16 MFMA in the same three terms, TP/NW pixels
    //      per wave, then sigmoid, rgb, masked-MSE partial, d rgb and sigmoid backward in fp32
    const int Kl = net.Kp[nl - 1];
    {
        const u16* Wh = reinterpret_cast<const u16*>(net.Wf[nl - 1]);
        const u16* Wl = Wh + (size_t)16 * Kl;
        constexpr int NJ = TP / NW / 16;
        f32x4 acc[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[j] = (f32x4){};
        const int ko = P::kofs16(lane);
        for (int k0 = 0; k0 < Kl; k0 += P::KS16) {
            const size_t wo = ((size_t)(k0 / P::KS16) * 64 + lane) * P::FE;
            const P::frag wh = P::load_frag(Wh + wo), wl = P::load_frag(Wl + wo);
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int px = wave * (TP / NW) + j * 16 + (lane & 15);
                const size_t bo = (size_t)px * lda + k0 + ko;
                const P::frag bh = P::load_frag(ah + bo), bl = P::load_frag(al + bo);
                acc[j] = P::mma16(wh, bh, acc[j]);
                acc[j] = P::mma16(wh, bl, acc[j]);
                acc[j] = P::mma16(wl, bh, acc[j]);
            }
        }
        if (lane < 16) {
            const float* bl = net.bias[nl - 1];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int px = wave * (TP / NW) + j * 16 + lane;
                const int p = p0 + px;
                if constexpr (FWD) {
                    if (p < Np) {
                        float* o = a.rgb + ((size_t)b * Np + p) * 3;
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            const float z = acc[j][c] + bl[c];
                            o[c] = 1.0f / (1.0f + expf(-z));
                        }
                    }
                } else {
                    float g[3] = {0.f, 0.f, 0.f};
                    float sq = 0.f, mv = 0.f;
                    const float4 tv = ld_as<float4>(&gl[px][0]);  // prefetched target, mask
                    const float tgt[3] = {tv.x, tv.y, tv.z};
                    if (p < Np) {
                        const float m = tv.w;
                        float* o = a.rgb ? a.rgb + ((size_t)b * Np + p) * 3 : nullptr;
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            const float z = acc[j][c] + bl[c];
                            const float y = 1.0f / (1.0f + expf(-z));
                            if (o) o[c] = y;
                            // model/planar.py:388-390 and its autograd: x = (p - g) m, d = 2 x m
                            const float x = (y - tgt[c]) * m;
                            sq += x * x;
                            const float d = (2.0f * x) * m;
                            g[c] = (d * (1.0f - y)) * y;  // torch sigmoid_backward
                        }
                        mv = m;
                    }
                    st_as<float4>(&gl[px][0], make_float4(g[0], g[1], g[2], 0.f));
#pragma unroll
                    for (int c = 0; c < 3; ++c) split1(g[c], gT[c][px], gT[4 + c][px]);
                    gT[3][px] = 0;
                    gT[7][px] = 0;
                    lsum[0][px] = sq;
                    lsum[1][px] = mv;
                }
            }
        }
    }
    if constexpr (!FWD) {
        __syncthreads();

        // ---- masked-MSE partial of the tile (fp64, fixed order) and the last bias gradient
        if (wave == 0) {
            double s0 = 0.0, s1 = 0.0;
            for (int px = lane; px < TP; px += 64) {
                s0 += (double)lsum[0][px];
                s1 += (double)lsum[1][px];
            }
            s0 = wave_total63(s0);
            s1 = wave_total63(s1);
            if (lane == 63) {
                a.loss_partial[2 * (size_t)blockIdx.x] = s0;
                a.loss_partial[2 * (size_t)blockIdx.x + 1] = s1;
            }
        } else if (wave == 1) {
            float s[3] = {0.f, 0.f, 0.f};
            for (int px = lane; px < TP; px += 64)
#pragma unroll
                for (int c = 0; c < 3; ++c) s[c] += gl[px][c];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float t = wave_total63(s[c]);
                if (lane == 63) a.blast_partial[(size_t)blockIdx.x * 3 + c] = t;
            }
        }

        // ---- last-layer weight gradient of the tile, as k_mlp_step: dW[c][k] = sum_px g[px][c]
        //      a_h[px][k]; A = g^T (rows 0-2 hi, rows 4-6 lo), B = the hi plane (transposed LDS read)
        {
            float* wout = a.wlast_partial + (size_t)blockIdx.x * 3 * Kl;
            const int g = lane >> 4, gi = lane & 15;
            for (int ct = wave; ct < Kl / 16; ct += NW) {
                f32x4 acc = (f32x4){};
#pragma unroll
                for (int k0 = 0; k0 < TP; k0 += 32) {
                    P::frag fa;
                    if (gi < 8) fa = P::load_frag(&gT[gi][k0 + 8 * g]);
                    else fa = (P::frag){};
                    const int r0 = k0 + 8 * g + (gi >> 2);
                    const u16* base = ah + (size_t)r0 * lda + ct * 16 + 4 * (gi & 3);
                    acc = P::mma16(fa, frag_of<P::frag>(tr_read16(base), tr_read16(base + 4 * lda)), acc);
                }
                // accumulator: lane l, reg r -> row 4 (l >> 4) + r, column l & 15: hi rows in lanes
                // 0-15, lo rows in lanes 16-31
                float lo[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) lo[c] = __shfl_down(acc[c], 16, 64);
                if (lane < 16) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) wout[(size_t)c * Kl + ct * 16 + lane] = acc[c] + lo[c];
                }
            }
        }
        __syncthreads();  // feat_{n-1} consumed

        // ---- d (last-layer input) operand: both planes' columns 0 .. Mt) = g split
        if ((int)threadIdx.x < TP) {
            const int i = threadIdx.x;
            const size_t at = (size_t)i * lda;
            const int Kt = net.Mt[nl - 1];
            for (int c = 0; c < Kt; ++c) {
                ah[at + c] = c < 3 ? gT[c][i] : (u16)0;
                al[at + c] = c < 3 ? gT[4 + c][i] : (u16)0;
            }
        }
        __syncthreads();

        // ---- dgrad chain, l = n-1 .. 1 : da = W_h^T dz_h + W_h^T dz_l + W_l^T dz_h; dz_l = da * relu'
        sth.clear();
        for (int l = nl - 1; l >= 1; --l) {
            const int R = net.Kp[l], Kk = net.Mt[l];
            f32x16 acc[RT][PT];
            const uint4 mw = *mask_record(a.mask_bits[l], blockIdx.x, wave, lane, NW);  // in flight behind the GEMM
            gemm_tile_split<RT, PT, NW>(acc, reinterpret_cast<const u16*>(net.Wt[l]), R, Kk, ah, al, lda, wave, lane, nullptr,
                                        sth, stl);
            __syncthreads();
            mask_epilogue_split<RT, PT, NW>(acc, ah, al, lda, R / 32, wave, lane, mw);
            __syncthreads();
            save_hi(a.dz[l], R);
        }

        // ---- layer-0 dgrad (three terms; dz_1's stores go out behind it) + posenc / warp adjoint in
        //      fp32 -> dH partial
        f32x16 acc[RT][PT];
        gemm_tile_split<RT, PT, NW>(acc, reinterpret_cast<const u16*>(net.Wt[0]), net.Kp[0], net.Mt[0], ah, al, lda, wave,
                                    lane, nullptr, sth, stl);
        __syncthreads();
        warp_adjoint_tail<P, TP, true, NW, false>(acc, net, a.geo, a.c2f.on, wsh, smem, wave, lane, b, p0, red, red9,
                                                  a.dH_partial, nullptr, nullptr, nullptr);
    }
}

}  // namespace marf

using namespace marf;

template <int TP, bool FWD>
static hipError_t launch_split(const StepArgs& a, size_t lds, int n_tiles, hipStream_t s) {
    hipError_t e = ensure_dynamic_lds((const void*)k_mlp_step_split<TP, FWD>, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_mlp_step_split<TP, FWD>), dim3(n_tiles), dim3(256), lds, s, a);
    return hipGetLastError();
}

// TP: 64 (hidden widths above 256) or 128; fwd_only: the render instantiation
hipError_t marf_launch_mlp_step_split(const StepArgs& a, int TP, bool fwd_only, size_t lds, int n_tiles, hipStream_t s) {
    if (TP == 64) return fwd_only ? launch_split<64, true>(a, lds, n_tiles, s) : launch_split<64, false>(a, lds, n_tiles, s);
    if (TP == 128) return fwd_only ? launch_split<128, true>(a, lds, n_tiles, s) : launch_split<128, false>(a, lds, n_tiles, s);
    return hipErrorInvalidValue;
}
