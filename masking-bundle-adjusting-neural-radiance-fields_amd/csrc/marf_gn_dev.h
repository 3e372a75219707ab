// marf_gn_dev.h -- the tile kernel of the Gauss-Newton normal equations of the registration problem on a frozen image
// (DESIGN.md §13).  With the image frozen, the B patches are independent 8-parameter non-linear
// least-squares problems; per patch b and real pixel q, with p the sigmoid output, g the target and
// m the mask,
//
//   r_qc = m_q (p_qc - g_qc)                     J_qc = m_q d p_qc / d vec(H_b)   (a row of 9, row-major)
//   sse_b = sum r^2    msum_b = sum m    g9_b = sum_qc J_qc^T r_qc    N_b = sum_qc J_qc^T J_qc
//
// One block = one tile of TP pixel slots, one template over the tile view (marf_gemm.h: a phase is
// written once over a view, a recipe is a view): TileView<PrecF32> (exact fp32 MFMA) and
// SplitView<false> (the bf16x3 tile recipe: three-term forward and dgrad).  Per tile:
//
//   prologue + forward as the warp-only tile step runs them (ReLU records to the scratch buffer, no
//   tile queued for saving) -> sigmoid: rgb, r_c, sigma'_c per slot
//   for c = 0, 1, 2:  step_fill_d with channel c alone (sigma'_c) -> the dgrad chain over the same
//                     records -> layer-0 dgrad -> posenc adjoint, stopped at the per-slot (du_c, dv_c)
//                     (warp_adjoint_tail's UV_ONLY) -> LDS [3][TP][2]
//   per slot: t_c = m (du_c, dv_c) d(u, v)/dX (the projective formulas of warp_adjoint_tail's dX0..dX2);
//   J_qc = t_c (x) (x, y, 1), so N += (sum_c t_c t_c^T) (x) (hom hom^T), g9 += (sum_c r_c t_c) (x) hom
//   56 values [sse, msum, g9 (9), N upper triangle row-major (45)] summed over the tile's slots in
//   fp64 in a fixed order (a value per wave at a time: lane-strided slots, then the DPP wave total),
//   one 56-value partial per tile.  A tile never straddles patches.
//
// k_gn_reduce then sums a patch's tile partials in fp64 in tile order.  No atomics anywhere: two
// launches on the same inputs give the same bits.  LOSS_ONLY runs the forward and sse / msum only --
// the same instructions up to there, so the same sse bits as the full launch.
//
// The kernel lives in this header because it is compiled in two units: marf_gn.hip instantiates the plain
// kernels (marf_gn_normal), marf_gn_robust.hip the ROBUST ones (marf_gn_normal_robust).  In one unit the
// second set of callers changed the inliner's view of the shared phases, and the plain full-launch
// kernels' register allocation moved with it; apart, the plain kernels' code is what it was.
#pragma once
#include "marf_gemm.h"

namespace marf {

constexpr int GN_VALS = 56;

// Prologue over the view: grid -> warp -> posenc (+ c2f) in fp32 with exact sincosf and the band
// weight multiplied in (what tile_prologue<PrecF32> and tile_prologue_split compute), each feature
// stored through the view (fp32, or split into bf16 hi + lo).  64 NW / TP threads share a pixel, the
// bands dealt round-robin.
template <int TP, int NW, class V>
MARF_DEV void gn_prologue(V v, const NetDev& net, const GeoDev& geo, int c2f_on, const float* wsh, int b, int p0) {
    constexpr int NPART = 64 * NW / TP;
    const int L = net.L;
    const int i = threadIdx.x % TP, part = threadIdx.x / TP;
    float x, y, uu = 0.f, vv = 0.f, X[3];
    slot_point<true>(geo, b, p0 + i, x, y, uu, vv, X);
    const typename V::Ref row = v.row(i);
    if (part == 0) {
        v.put(row + 0, uu);
        v.put(row + 1, vv);
    }
    for (int q = part; q < 2 * L; q += NPART) {
        const int c = q >= L, k = q - c * L;
        float s, co;
        band_sincos<false>(c ? vv : uu, k, s, co);
        if (c2f_on) {
            const float w = wsh[k];
            s = s * w;
            co = co * w;
        }
        v.put(row + (2 + 2 * c * L + k), s);
        v.put(row + (2 + 2 * c * L + L + k), co);
    }
    for (int f = net.D + part; f < net.Kp[0]; f += NPART) v.zero(row + f);
}

// Per slot of the wave's 16-pixel groups (lanes 0 - 15; acc = last_layer_gemm's): sigmoid, rgb, the
// masked residual r_c = (p_c - g_c) m and sigma'_c = (1 - p_c) p_c -> rs [r (3), 0, sigma' (3), m];
// lsum: sum_c r_c^2 and m (padding slots: zeros).
// ROBUST (iteratively reweighted least squares): with e = sum_c r_c^2 and the scale delta, the loss rho(e)
// goes to lsum[0] in e's place and the stored r_c and m are scaled by sqrt(w), w = rho'(e) -- Huber: rho
// = e, w = 1 up to delta^2, beyond it 2 delta sqrt(e) - delta^2, delta / sqrt(e); Cauchy: delta^2 log1p(e
// / delta^2), 1 / (1 + e / delta^2) -- so everything downstream sums w J^T r and w J^T J; lsum[1] keeps
// the unscaled m.  w = 1 scales by sqrt(1) = 1: the plain launch's bits.  w of a real pixel -> ga.weight.
template <int TP, int NW, int NJ, int TS, bool ROBUST>
MARF_DEV void gn_slots(const GnArgs& ga, const f32x4 (&acc)[NJ], int wave, int lane, int b, int p0,
                       const float (&gl)[TP][4], float (&lsum)[2][TP], float (&rs)[TS][8]) {
    const StepArgs& a = ga.s;
    const int Np = a.geo.Np;
    if (lane < 16) {
        const float* bl = a.net.bias[a.net.n_layers - 1];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int px = wave * (TP / NW) + j * 16 + lane;
            const int p = p0 + px;
            float r[3] = {0.f, 0.f, 0.f}, sg[3] = {0.f, 0.f, 0.f};
            float sq = 0.f, mv = 0.f, ms = 0.f;  // ms: the m the Jacobian carries (ROBUST: sqrt(w) m)
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
                    const float x = (y - tgt[c]) * m;
                    sq += x * x;
                    r[c] = x;
                    sg[c] = (1.0f - y) * y;
                }
                mv = m;
                ms = m;
                if constexpr (ROBUST) {
                    const float delta = ga.robust_delta, d2 = delta * delta;
                    float w = 1.0f;
                    if (ga.robust_kind == GN_HUBER) {
                        if (sq > d2) {
                            const float s = sqrtf(sq);
                            w = delta / s;
                            sq = 2.0f * delta * s - d2;
                        }
                    } else {
                        const float q = sq / d2;
                        w = 1.0f / (1.0f + q);
                        sq = d2 * log1pf(q);
                    }
                    const float sw = sqrtf(w);
#pragma unroll
                    for (int c = 0; c < 3; ++c) r[c] *= sw;
                    ms = m * sw;
                    if (ga.weight) ga.weight[(size_t)b * Np + p] = w;
                }
            }
            lsum[0][px] = sq;
            lsum[1][px] = mv;
            if constexpr (TS == TP) {
                st_as<float4>(&rs[px][0], make_float4(r[0], r[1], r[2], 0.f));
                st_as<float4>(&rs[px][4], make_float4(sg[0], sg[1], sg[2], ms));
            }
        }
    }
}

// One of the tile's 56 values: term(px) summed over the slots in fp64 -- lane-strided, then the DPP
// wave total (fixed order) -- by one wave.
template <int TP, class F>
MARF_DEV void gn_tile_sum(double* out, int lane, F term) {
    double s = 0.0;
    for (int px = lane; px < TP; px += 64) s += (double)term(px);
    s = wave_total63(s);
    if (lane == 63) *out = s;
}

// One block per CU either way (the tile takes 131 - 135 KB of LDS).  The split view may use all 512
// registers of a wave; the fp32 view is held to k_mlp_step's 256 (two blocks' worth): at 512 its
// accumulators went to the accumulator half, which the epilogues' VALU cannot read, and 516 B per lane
// of scratch came with the copies.  ROBUST: gn_slots' per-pixel weight between the residuals and the
// sums (marf_gn_normal_robust); off, the kernel is marf_gn_normal's.
template <class V, int TP, bool LOSS_ONLY, bool ROBUST = false>
__global__ __launch_bounds__(256, V::SPLIT ? 1 : 2) void k_gn(GnArgs ga) {
    typedef typename V::P P;
    constexpr int NW = 4;
    constexpr int PT = TP / 32;
    constexpr int RT = 8 / PT;
    constexpr int NJ = TP / NW / 16;
    constexpr int TS = LOSS_ONLY ? 1 : TP;  // the full launch's arrays
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float wsh[32];
    __shared__ float red[LOSS_ONLY ? 1 : 64 * NW * 2];        // the posenc adjoint's shares per part
    __shared__ __attribute__((aligned(16))) float gl[TP][4];  // target + mask, then the chain's start d
    __shared__ float lsum[2][TP];                              // per-slot sum_c r_c^2 (ROBUST: rho) and m
    __shared__ __attribute__((aligned(16))) float rs[TS][8];  // r_c (3), 0, sigma'_c (3), m
    __shared__ float duv[3][TS][2];                            // (du_c, dv_c) per channel and slot
    __shared__ float sq[TS][12];                               // sum_c t_c t_c^T (6), sum_c r_c t_c (3), hom (3)

    const StepArgs& a = ga.s;
    const NetDev& net = a.net;
    V v(smem, a.lda, TP);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int b, p0;
    long long slot0;
    tile_origin(a.geo, blockIdx.x, TP, b, p0, slot0);
    const int nl = net.n_layers;
    double* part = ga.partial + (size_t)blockIdx.x * GN_VALS;

    if ((int)threadIdx.x < net.L) wsh[threadIdx.x] = a.c2f_w[threadIdx.x];
    const float4 tg = step_target<TP>(a, b, p0);
    __syncthreads();
    gn_prologue<TP, NW>(v, net, a.geo, a.c2f.on, wsh, b, p0);
    if ((int)threadIdx.x < TP) st_as<float4>(&gl[threadIdx.x][0], tg);
    __syncthreads();

    // ---- hidden layers (forward); nothing is queued for saving, the ReLU records go to the scratch
    for (int l = 0; l < nl - 1; ++l) {
        const int K = net.Kp[l], M = net.Mp[l];
        f32x16 acc[RT][PT];
        v.template gemm<RT, PT, NW>(acc, net.Wf[l], M, K, net.bias[l], wave, lane);
        __syncthreads();  // every wave has consumed the layer input
        relu_epilogue<RT, PT, NW>(acc, v, M / 32, wave, lane, LOSS_ONLY ? nullptr : a.mask_bits[l + 1], blockIdx.x);
        __syncthreads();
    }

    // ---- last layer, sigmoid, residuals; sse and msum of the tile
    {
        f32x4 acc[NJ];
        last_layer_gemm<TP, NW>(v, net.Wf[nl - 1], net.Kp[nl - 1], wave, lane, acc);
        gn_slots<TP, NW, NJ, TS, ROBUST>(ga, acc, wave, lane, b, p0, gl, lsum, rs);
    }
    __syncthreads();  // feat_{n-1} consumed
    if (wave == 0) {
        gn_tile_sum<TP>(part + 0, lane, [&](int px) { return lsum[0][px]; });
        gn_tile_sum<TP>(part + 1, lane, [&](int px) { return lsum[1][px]; });
    }
    if constexpr (!LOSS_ONLY) {
        // ---- one pass down the chain per output channel: d p_c / d (u, v) per slot
        for (int c = 0; c < 3; ++c) {
            if ((int)threadIdx.x < TP) {  // (step_fill_d reads the thread's own row: no barrier between)
                const float s = rs[threadIdx.x][4 + c];
                st_as<float4>(&gl[threadIdx.x][0], make_float4(c == 0 ? s : 0.f, c == 1 ? s : 0.f, c == 2 ? s : 0.f, 0.f));
            }
            step_fill_d<TP>(v, gl, net.Mt[nl - 1], 0);
            __syncthreads();
            for (int l = nl - 1; l >= 1; --l) {
                const int R = net.Kp[l], Kk = net.Mt[l];
                f32x16 acc[RT][PT];
                const uint4 mw = *mask_record(a.mask_bits[l], blockIdx.x, wave, lane, NW);  // in flight behind the GEMM
                v.template gemm<RT, PT, NW>(acc, net.Wt[l], R, Kk, nullptr, wave, lane);
                __syncthreads();
                mask_epilogue<RT, PT, NW>(acc, v, R / 32, wave, lane, mw);
                __syncthreads();
            }
            f32x16 acc[RT][PT];
            v.template gemm<RT, PT, NW>(acc, net.Wt[0], net.Kp[0], net.Mt[0], nullptr, wave, lane);
            __syncthreads();
            // the step's tail, stopped at the per-slot (du, dv) (UV_ONLY): -> duv[c]
            warp_adjoint_tail<P, TP, true, NW, false, RT, PT, true>(acc, net, a.geo, a.c2f.on, wsh, smem, wave, lane, b, p0, red,
                                                                    nullptr, nullptr, &duv[c][0][0], nullptr, nullptr);
            __syncthreads();  // the df image (the tile) and red are free for the next channel
        }

        // ---- per slot: t_c = m (du_c, dv_c) d(u, v)/dX; (u, v) = X[:2] / (X[2] + 1e-8)
        if ((int)threadIdx.x < TP) {
            const int i = threadIdx.x;
            float x = 0.f, y = 0.f, uu = 0.f, vv = 0.f, X[3] = {0.f, 0.f, 1.f};
            const bool valid = slot_point<true>(a.geo, b, p0 + i, x, y, uu, vv, X);
            float S[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, w[3] = {0.f, 0.f, 0.f};
            if (valid) {
                const float m = rs[i][7];
                const float dd = X[2] + 1e-8f;
                const float dd2 = dd * dd;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float du = duv[c][i][0], dv = duv[c][i][1];
                    const float t0 = (du / dd) * m, t1 = (dv / dd) * m;
                    const float t2 = ((-du * X[0]) / dd2 + (-dv * X[1]) / dd2) * m;
                    const float r = rs[i][c];
                    S[0] += t0 * t0;
                    S[1] += t0 * t1;
                    S[2] += t0 * t2;
                    S[3] += t1 * t1;
                    S[4] += t1 * t2;
                    S[5] += t2 * t2;
                    w[0] += r * t0;
                    w[1] += r * t1;
                    w[2] += r * t2;
                }
            }  // (a padding slot: zeros, hom = (0, 0, 1))
#pragma unroll
            for (int e = 0; e < 6; ++e) sq[i][e] = S[e];
#pragma unroll
            for (int e = 0; e < 3; ++e) sq[i][6 + e] = w[e];
            sq[i][9] = x;
            sq[i][10] = y;
            sq[i][11] = 1.f;
        }
        __syncthreads();

        // ---- the tile's g9 and N: value e = 2 + wave + 4 k by wave `wave`
        for (int e = 2 + wave; e < GN_VALS; e += NW) {
            if (e < 11) {  // g9[3 r + i] = w[r] hom[i]
                const int r = (e - 2) / 3, i = (e - 2) - 3 * r;
                gn_tile_sum<TP>(part + e, lane, [&](int px) { return sq[px][6 + r] * sq[px][9 + i]; });
            } else {  // N[row][col], row <= col, row = 3 r + i, col = 3 s + j: S[r][s] hom[i] hom[j]
                int idx = e - 11, row = 0;
                while (idx >= 9 - row) {
                    idx -= 9 - row;
                    ++row;
                }
                const int col = row + idx;
                const int r = row / 3, i = row - 3 * r, s = col / 3, j = col - 3 * s;
                const int si = r == 0 ? s : (r == 1 ? 2 + s : 5);  // (r, s), r <= s, in S's upper triangle
                gn_tile_sum<TP>(part + e, lane, [&](int px) { return sq[px][si] * (sq[px][9 + i] * sq[px][9 + j]); });
            }
        }
    }
}

template <class V, int TP, bool ROBUST>
static hipError_t launch_gn(const GnArgs& a, bool loss_only, size_t lds, int n_tiles, hipStream_t s) {
    const void* k = loss_only ? (const void*)k_gn<V, TP, true, ROBUST> : (const void*)k_gn<V, TP, false, ROBUST>;
    hipError_t e = ensure_dynamic_lds(k, lds);
    if (e != hipSuccess) return e;
    if (loss_only) hipLaunchKernelGGL((k_gn<V, TP, true, ROBUST>), dim3(n_tiles), dim3(256), lds, s, a);
    else hipLaunchKernelGGL((k_gn<V, TP, false, ROBUST>), dim3(n_tiles), dim3(256), lds, s, a);
    return hipGetLastError();
}

template <bool ROBUST>
static hipError_t pick_gn(const GnArgs& a, bool split, int TP, bool loss_only, size_t lds, int n_tiles, hipStream_t s) {
    if (split && TP == 128) return launch_gn<SplitView<false>, 128, ROBUST>(a, loss_only, lds, n_tiles, s);
    if (split && TP == 64) return launch_gn<SplitView<false>, 64, ROBUST>(a, loss_only, lds, n_tiles, s);
    if (!split && TP == 64) return launch_gn<TileView<PrecF32>, 64, ROBUST>(a, loss_only, lds, n_tiles, s);
    return hipErrorInvalidValue;
}

}  // namespace marf
