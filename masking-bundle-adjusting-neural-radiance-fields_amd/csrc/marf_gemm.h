// marf_gemm.h -- device building blocks shared by the per-tile MLP kernels (marf_mlp.hip,
// marf_step.hip, marf_step_split.hip, marf_mask.hip): the LDS-resident activation tile GEMM
// (weights = MFMA A operand streamed from L2, activations = B operand read from LDS), plain and
// all-operands-split, tile addressing, and the per-tile phases.
//
// The rule: a phase is written once, over a view of the tile (TileView<P>: one plane of P::T;
// SplitView<BOTH>: two u16 planes, hi then lo -- "tile views" below); a recipe is a view.  Written
// over the views: the ReLU / dgrad epilogues, the last layer's forward, the loss tail of the fused
// step.  (The dgrad chain's loop -- record load, gemm, barrier, epilogue, barrier, queue_save -- is
// five lines over the view in each kernel: stamps, the skip epilogue and the save differ.)  Not
// shared, on purpose: tile_prologue against marf_step_split.hip's tile_prologue_split
// (different band dealing and sincos) and gemm_rows against gemm_rows_split (different pipelines).
//
// Orientation: Z^T[out x px] = W[out x in] . A^T[in x px]: lane = output row / 8 contiguous k for
// the weights, lane = pixel / 8 contiguous features for the activations; the accumulator holds a
// pixel per lane and features in registers.  256 threads = 4 waves; output row tiles (32) of a
// layer are dealt round-robin to the 4 waves, each wave covers all PT = TP/32 pixel tiles.
#pragma once
#include <type_traits>

#include "marf_args.h"

namespace marf {

// Transposed LDS read (gfx950 ds_read_b64_tr_b16): per 16-lane group, a 4 x 16 block of bf16 is
// read row-major (lane gi addresses row gi >> 2, columns 4 (gi & 3) ..) and delivered
// column-major: lane gi receives column gi of the 4 rows.
MARF_DEV i16x4 tr_read16(const u16* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) i16x4*)(p));
}

template <class P>
MARF_DEV void copy_tile_out(const typename P::T* act, int lda, int rows, int cols, typename P::T* dst, int ldd,
                            int rmode = 0) {
    // LDS [rows][lda] -> global [rows][ldd], first `cols` columns. bf16: 16-byte chunks.
    // The (row, chunk) walk is incremental: one division per call, none per element.
    typedef typename P::T T;
    if (sizeof(T) == 2) {
        const int nch = cols / 8;
        const int step = blockDim.x, dr = step / nch, dc = step - dr * nch;
        int r = threadIdx.x / nch, c = threadIdx.x - r * nch;
        for (; r < rows;) {
            st_as<uint4>(dst + (size_t)r * ldd + 8 * c, ld_as<uint4>(act + (size_t)r * lda + 8 * c));
            r += dr;
            c += dc;
            if (c >= nch) {
                c -= nch;
                ++r;
            }
        }
    } else {
        for (int e = threadIdx.x; e < rows * cols; e += blockDim.x) {
            int r = e / cols, c = e - r * cols;
            dst[(size_t)r * ldd + c] = rmode ? diag_round(act[(size_t)r * lda + c], rmode) : act[(size_t)r * lda + c];
        }
    }
}

// Streams an LDS tile [rows][lda] (first `cols` columns) to global [rows][ldd] in 16-byte chunks
// right after the GEMM that reads the tile (gemm_tile flushes it there, before the epilogue
// rewrites the tile).  gemm_rows can also interleave the chunks with its k-steps (JOB 1 / 2), but
// vmcnt retires in issue order, so a store between the weight-fragment loads makes every later
// fragment wait for it: measured slower (C5 80.7 vs 66.7 ms), kept only as the JOB template.
// bf16 tiles only (16-B aligned LDS rows).
//
// Wave-uniform walk: rpi = 64 / nch whole rows per wave step (lane -> row lane / nch, chunk
// lane % nch); wave w of nw copies row groups w, w + nw, ...
template <class T>
struct TileStore {
    T* dst;
    int lda, ldd, rows, rpi, q, nq, wave, nw;
    int lr, lc;  // per lane
    bool active;

    MARF_DEV void clear() {
        active = false;
        q = nq = 0;
    }
    MARF_DEV void init(int lda_, T* d, int ldd_, int rows_, int cols, int wave_, int lane, int nw_ = 4) {
        constexpr int VEC = 16 / sizeof(T);
        const int nch = cols / VEC;  // <= 64 (cols <= 512)
        dst = d;
        lda = lda_;
        ldd = ldd_;
        rows = rows_;
        wave = wave_;
        nw = nw_;
        rpi = 64 / nch;
        lr = lane / nch;
        lc = lane - lr * nch;
        q = 0;
        nq = (rows + nw * rpi - 1) / (nw * rpi);
        active = true;
    }
    MARF_DEV int row() const {
        const int qq = q < nq ? q : nq - 1;
        const int r = (qq * nw + wave) * rpi + lr;
        return r < rows ? r : rows - 1;  // idle lanes / surplus rows repeat the last row's chunk
    }
    MARF_DEV uint4 read(const T* src) const {
        constexpr int VEC = 16 / sizeof(T);
        return ld_as<uint4>(src + (size_t)row() * lda + VEC * lc);
    }
    MARF_DEV void write(uint4 v) {
        constexpr int VEC = 16 / sizeof(T);
        st_as<uint4>(dst + (size_t)row() * ldd + VEC * lc, v);
        ++q;
    }
    MARF_DEV void flush(const T* src) {
        while (q < nq) write(read(src));
    }
};

// acc[i][PT] += W[rows (wave + NW i)*32 .., k] . act[px, k]^T over k < K for the NA row tiles this
// wave owns (i < NA; NW waves per block deal the row tiles round-robin).  NA is dispatched once per layer (wave-uniform), so the body is branch-free.
//
// Schedule: the weight fragments stream from L2 through a static 4-deep register ring (slot u is
// reloaded for k-step k+4 right after its MFMAs issue: three k-steps of latency cover, no register
// moves), the activation fragments of step k+1 are read from LDS while step k's MFMAs run (two
// statically named buffers).  Loads past the last k-step are clamped to it (harmless L2 hits).
// JOB: one TileStore chunk per k-step (1) or per second k-step (2: the job has at most half as many
// chunks as the GEMM k-steps, e.g. a 512-wide tile saved during a 512-deep GEMM at 8 waves, where
// one chunk per k-step would rewrite the last chunk for half the GEMM), read before the B
// prefetch, stored after the A reload.
template <class P, int NA, int RT, int PT, int JOB, int NW = 4>
MARF_DEV void gemm_rows(f32x16 (&acc)[RT][PT], const typename P::T* __restrict__ W, int K,
                        const typename P::T* act, int lda, int wave, int lane, TileStore<typename P::T>& st) {
    typedef typename P::frag F;
    const int ko = P::kofs(lane);
    const int rl = lane & 31;
    const int nk = K / P::KS;
    // fragment-major weights (marf_common.h): fragment (rt, ks) at ((rt * nk + ks) * 64 + lane) * FE
    const typename P::T* wrow[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) wrow[i] = W + ((size_t)(wave + NW * i) * nk * 64 + lane) * P::FE;
    const typename P::T* brow = act + (size_t)rl * lda + ko;
    auto ldA = [&](F (&dst)[NA], int k) {
        const int kc = (k < nk ? k : nk - 1) * 64 * P::FE;
#pragma unroll
        for (int i = 0; i < NA; ++i) dst[i] = P::load_frag(wrow[i] + kc);
    };
    auto ldB = [&](F (&dst)[PT], int k) {
        const int kc = (k < nk ? k : nk - 1) * P::KS;
#pragma unroll
        for (int j = 0; j < PT; ++j) dst[j] = P::load_frag(brow + (size_t)j * 32 * lda + kc);
    };
    auto mma = [&](const F (&a)[NA], const F (&b)[PT]) {
#pragma unroll
        for (int j = 0; j < PT; ++j)
#pragma unroll
            for (int i = 0; i < NA; ++i) acc[i][j] = P::mma32(a[i], b[j], acc[i][j]);
    };
    uint4 sv = make_uint4(0, 0, 0, 0);
    // pos: the k-step's position in the 4-step unrolled body (0 in the 2-deep-ring body, which
    // places the job at positions 0 and 1 of its 2-step iterations)
    auto sread = [&](auto posc) {
        if constexpr (JOB == 1 || (JOB == 2 && decltype(posc)::value % 2 == 0)) sv = st.read(act);
    };
    auto swrite = [&](auto posc) {
        if constexpr (JOB == 1 || (JOB == 2 && decltype(posc)::value % 2 == 0)) st.write(sv);
    };
    typedef std::integral_constant<int, 0> J0;
    typedef std::integral_constant<int, 1> J1;
    typedef std::integral_constant<int, 2> J2;
    typedef std::integral_constant<int, 3> J3;
    F A0[NA], A1[NA], A2[NA], A3[NA], B0[PT], B1[PT];
    if constexpr (sizeof(F) * NA > 32) {
        // wide row blocks (bf16, NA > 2): a 2-deep ring keeps the kernel inside 256 VGPRs
        ldA(A0, 0);
        ldA(A1, 1);
        ldB(B0, 0);
        int k = 0;
        for (; k + 2 <= nk; k += 2) {
            sread(J0());
            ldB(B1, k + 1);
            __builtin_amdgcn_sched_barrier(0);
            mma(A0, B0);
            __builtin_amdgcn_sched_barrier(0);
            ldA(A0, k + 2);
            swrite(J0());
            sread(J1());
            ldB(B0, k + 2);
            __builtin_amdgcn_sched_barrier(0);
            mma(A1, B1);
            __builtin_amdgcn_sched_barrier(0);
            ldA(A1, k + 3);
            swrite(J1());
        }
        if (k < nk) mma(A0, B0);
        if constexpr (JOB) st.flush(act);
        return;
    }
    ldA(A0, 0);
    ldA(A1, 1);
    ldA(A2, 2);
    ldA(A3, 3);
    ldB(B0, 0);
    int k = 0;
    // sched_barrier pins the issue order: left alone, the scheduler sinks every weight load to
    // the loop end (one MFMA of latency cover) and folds the two B buffers into one.
    for (; k + 4 <= nk; k += 4) {
        sread(J0());
        ldB(B1, k + 1);
        __builtin_amdgcn_sched_barrier(0);
        mma(A0, B0);
        __builtin_amdgcn_sched_barrier(0);
        ldA(A0, k + 4);
        swrite(J0());
        sread(J1());
        ldB(B0, k + 2);
        __builtin_amdgcn_sched_barrier(0);
        mma(A1, B1);
        __builtin_amdgcn_sched_barrier(0);
        ldA(A1, k + 5);
        swrite(J1());
        sread(J2());
        ldB(B1, k + 3);
        __builtin_amdgcn_sched_barrier(0);
        mma(A2, B0);
        __builtin_amdgcn_sched_barrier(0);
        ldA(A2, k + 6);
        swrite(J2());
        sread(J3());
        ldB(B0, k + 4);
        __builtin_amdgcn_sched_barrier(0);
        mma(A3, B1);
        __builtin_amdgcn_sched_barrier(0);
        ldA(A3, k + 7);
        swrite(J3());
    }
    // remainder (nk % 4 steps): A0..A2 hold steps k..k+2, B0 holds step k
    if (k < nk) {
        ldB(B1, k + 1);
        mma(A0, B0);
        if (k + 1 < nk) {
            ldB(B0, k + 2);
            mma(A1, B1);
            if (k + 2 < nk) mma(A2, B0);
        }
    }
    if constexpr (JOB) st.flush(act);
}

// Accumulators start at the bias of their output row when `bias` is given (so the epilogue does
// not add it), else at zero.
template <class P, int RT, int PT, int NW = 4>
MARF_DEV void gemm_tile(f32x16 (&acc)[RT][PT], const typename P::T* __restrict__ W, int K, int n_rt,
                        const typename P::T* act, int lda, int wave, int lane, const float* bias,
                        TileStore<typename P::T>& st) {
#pragma unroll
    for (int i = 0; i < RT; ++i) {
        f32x16 init = (f32x16){};
        const int rt = wave + NW * i;
        if (bias && rt < n_rt) {
            const float* bb = bias + rt * 32 + 4 * (lane >> 5);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 bv = ld_as<float4>(bb + 8 * q);
                init[4 * q] = bv.x;
                init[4 * q + 1] = bv.y;
                init[4 * q + 2] = bv.z;
                init[4 * q + 3] = bv.w;
            }
        }
#pragma unroll
        for (int j = 0; j < PT; ++j) acc[i][j] = init;
    }
    int na = (n_rt - wave + NW - 1) / NW;
    na = na < 0 ? 0 : (na > RT ? RT : na);
    // The saved tile's stores go out after the GEMM instead of between its weight-fragment loads:
    // vmcnt retires in issue order, so each fragment wait also waited for the stores issued before
    // it.  Same bits; C5 (8-wave block) 80.7 -> 66.7 ms, plain bf16 at C3 (4-wave) 5.21 -> 5.07 ms
    // (profiles/r4w, r4x).  The stores drain during the epilogue, which loads nothing.
    switch (na) {
        case 1: gemm_rows<P, 1, RT, PT, 0, NW>(acc, W, K, act, lda, wave, lane, st); break;
        case 2: gemm_rows<P, 2, RT, PT, 0, NW>(acc, W, K, act, lda, wave, lane, st); break;
        case 3: if constexpr (RT >= 3) gemm_rows<P, 3, RT, PT, 0, NW>(acc, W, K, act, lda, wave, lane, st); break;
        case 4: if constexpr (RT >= 4) gemm_rows<P, 4, RT, PT, 0, NW>(acc, W, K, act, lda, wave, lane, st); break;
        default: break;
    }
    if (st.active) st.flush(act);
}

// Store 4 consecutive rows (features) of one accumulator group for this lane's pixel.
template <class P>
MARF_DEV void store4(typename P::T* dst, float x0, float x1, float x2, float x3) {
    if constexpr (sizeof(typename P::T) == 2) {
        uint2 v;  // one packed RNE conversion per pair
        v.x = P::pk2(x0, x1);
        v.y = P::pk2(x2, x3);
        st_as<uint2>(dst, v);
    } else {
        dst[0] = x0;
        dst[1] = x1;
        dst[2] = x2;
        dst[3] = x3;
    }
}

MARF_DEV void tile_origin(const GeoDev& g, int tile, int TP, int& b, int& p0, long long& slot0) {
    int tpp = g.Np_pad / TP;
    b = tile / tpp;
    p0 = (tile - b * tpp) * TP;
    slot0 = (long long)b * g.Np_pad + p0;
}


// Save the LDS tile to global: bf16 tiles stream during the GEMM that follows (job handed to
// gemm_tile), fp32 tiles (unaligned LDS rows) are copied right away (job left idle).
template <class P, int NW = 4>
MARF_DEV void save_tile(TileStore<typename P::T>& job, const typename P::T* act, int lda, int rows, int cols,
                        typename P::T* dst, int rmode = 0) {
    if constexpr (sizeof(typename P::T) == 2) {
        const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        job.init(lda, dst, cols, rows, cols, wave, lane, NW);
    } else {
        copy_tile_out<P>(act, lda, rows, cols, dst, cols, rmode);  // (rmode: MARF_DIAG_RT experiments)
        job.clear();
    }
}

// ======================================================================== per-tile phases

// BARF coarse-to-fine weight of every band into LDS (model/planar.py:462-470); 1 without c2f.
MARF_DEV void c2f_weights_lds(const C2fDev& c2f, int L, float* wsh) {
    if ((int)threadIdx.x < L)
        wsh[threadIdx.x] = c2f.on ? c2f_weight(*c2f.progress, c2f.start, c2f.span, L, threadIdx.x) : 1.0f;
}

// Prologue: pixel grid -> sl(3) warp -> posenc (+c2f) of the tile's TP slots -> act [TP][Kp0]
// (warp.py:33-81, model/planar.py:451-471; feature layout [u, v, sin_k(u), cos_k(u), sin_k(v),
// cos_k(v)], zero padded to Kp0).  NPART = 64 NW / TP threads share a pixel: half of them take u,
// half v, each a contiguous run of bands, written as bf16 pairs (one 4-byte LDS store per pair).
// c0: the first column (a skip layer's posenc block, written again at column Mp[l-1]; even).
template <class P, int TP, bool GRID_ONLY = false, int NW = 4>
MARF_DEV void tile_prologue(const NetDev& net, const GeoDev& geo, int c2f_on, const float* wsh,
                            typename P::T* act, int lda, int b, int p0, int c0 = 0) {
    typedef typename P::T T;
    constexpr int NPART = 64 * NW / TP, HALF = NPART / 2;
    const int L = net.L;
    const int i = threadIdx.x % TP, part = threadIdx.x / TP;
    float x, y, u = 0.f, v = 0.f, X[3];
    slot_point<GRID_ONLY>(geo, b, p0 + i, x, y, u, v, X);
    T* row = act + (size_t)i * lda + c0;
    auto put2 = [&](int col, float a0, float a1) {  // col even
        if constexpr (sizeof(T) == 2) {
            st_as<uint32_t>(row + col, P::pk2(a0, a1));
        } else {
            row[col] = a0;
            row[col + 1] = a1;
        }
    };
    if (part == NPART - 1) put2(0, MARF_DIAG_ROUND(u, net.diag[0], 2), MARF_DIAG_ROUND(v, net.diag[0], 2));
    if (L > 0) {
        const int c = part / HALF, sub = part - c * HALF;
        const float cv = c ? v : u;
        const int k0 = sub * L / HALF, k1 = (sub + 1) * L / HALF;
        const int cs = 2 + 2 * c * L, cc = cs + L;  // first sin / cos column of coordinate c
        int k = k0;
        auto band = [&](int kk, float& sv, float& cvv) {
            band_sincos<sizeof(T) == 2>(cv, kk, sv, cvv);
            if (c2f_on) {
                const float w = wsh[kk];
                sv = sv * w;
                cvv = cvv * w;
            }
            sv = MARF_DIAG_ROUND(sv, net.diag[0], 2);
            cvv = MARF_DIAG_ROUND(cvv, net.diag[0], 2);
        };
        if ((k & 1) && k < k1) {  // odd start: single band
            float s0, c0;
            band(k, s0, c0);
            row[cs + k] = P::cvt(s0);
            row[cc + k] = P::cvt(c0);
            ++k;
        }
        for (; k + 1 < k1; k += 2) {
            float s0, c0, s1, c1;
            band(k, s0, c0);
            band(k + 1, s1, c1);
            if ((cs & 1) == 0) {
                put2(cs + k, s0, s1);
            } else {
                row[cs + k] = P::cvt(s0);
                row[cs + k + 1] = P::cvt(s1);
            }
            if (((cc + k) & 1) == 0) {
                put2(cc + k, c0, c1);
            } else {
                row[cc + k] = P::cvt(c0);
                row[cc + k + 1] = P::cvt(c1);
            }
        }
        if (k < k1) {
            float s0, c0;
            band(k, s0, c0);
            row[cs + k] = P::cvt(s0);
            row[cc + k] = P::cvt(c0);
        }
    }
    for (int f = net.D + 2 * part; f < net.Kp[0]; f += 2 * NPART) put2(f, 0.f, 0.f);  // D, Kp0 even
}

// ReLU mask records: one uint4 per lane per (tile, layer) at ((tile * 4 + wave) * 64 + lane), i.e.
// one contiguous 1 KB wave burst.  The RT x PT accumulator tiles of a wave are numbered
// ti = i * PT + j (<= 8); tile ti's 16 bits live in word ti >> 1, bits 16 (1 - (ti & 1)) + 15 - r
// for accumulator register r.  The dgrad epilogue of the backward finds the same (feature, pixel)
// in the same wave / lane / register (gemm_tile deals row tiles identically for W and W^T).
// (uint4 is these buffers' element type: every access to them is a whole record through here.)
MARF_DEV uint4* mask_record(uint64_t* mk, int tile, int wave, int lane, int nw = 4) {
    return reinterpret_cast<uint4*>(mk) + ((size_t)tile * nw + wave) * 64 + lane;
}

// Skip layer's dgrad rows past its feature input (rows rt_lo * 32 .. n_rt * 32 = the posenc block,
// model/planar.py:440-441): no ReLU, the gradient of the posenc features, added into the fp32
// accumulator dsk [TP][Kp0] (one (pixel, feature) per lane and register: no two lanes share one).
template <class P, int RT, int PT, int NW = 4>
MARF_DEV void skip_epilogue(const f32x16 (&acc)[RT][PT], float* dsk, int kp0, int rt_lo, int n_rt, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < RT; ++i) {
        const int rt = wave + NW * i;
        if (rt < rt_lo || rt >= n_rt) continue;
#pragma unroll
        for (int j = 0; j < PT; ++j) {
            const int px = j * 32 + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int f = (rt - rt_lo) * 32 + acc_row(lane, r);
                dsk[(size_t)px * kp0 + f] += acc[i][j][r];
            }
        }
    }
}

// LDS byte offset of the skip accumulator dsk: past the activation tile and the fp32 df image
template <class P, int TP>
MARF_DEV int skip_lds_off(const NetDev& net, int lda) {
    const int a = TP * lda * (int)sizeof(typename P::T), d = TP * (net.Kp[0] + 1) * 4;
    return ((a > d ? a : d) + 15) & ~15;
}

// Layer-0 dgrad (d feat_0 = W_0^T dz_1, act holds dz_1) and the posenc / projective-warp adjoint
// (model/planar.py:451-471, warp.py:74-78 backward): per slot d(u, v), then for the grid geometry
// d(Hx) and one dH[3x3] partial per tile (fixed-order wave + block sums); for explicit coordinates
// d coords.  `red` needs 64 NW * 2 floats, `red9` NW * 9.  smem = the act tile (reused as fp32).
// dsk: the skip layers' posenc gradient ([TP][Kp0] fp32, added to d feat_0), or null.
// warp_adjoint_tail: everything after the layer-0 dgrad GEMM (acc = d feat_0, every wave past the
// barrier that follows the GEMM), shared with the split tile step, which runs its own three-term
// GEMM.  FAST: the posenc sin / cos of the 16-bit prologue (band_sincos).
// UV_ONLY: the tail stops at the per-slot (du, dv), written for every slot of the tile to
// d_coords[2 slot] (a tile-local [TP][2] image, LDS or global; no barrier behind it) -- the
// Gauss-Newton kernel (marf_gn.hip), which runs the tail once per output channel; no dH, red9 unused.
template <class P, int TP, bool GRID_ONLY, int NW, bool FAST, int RT, int PT, bool UV_ONLY = false>
MARF_DEV void warp_adjoint_tail(const f32x16 (&acc)[RT][PT], const NetDev& net, const GeoDev& geo, int c2f_on,
                                const float* wsh, char* smem, int wave, int lane, int b, int p0, float* red,
                                float* red9, float* dH_partial, float* d_coords, unsigned long long* sp,
                                const float* dsk) {
    const int L = net.L;
    const int R = net.Kp[0], n_rt = R / 32;
    float* df = reinterpret_cast<float*>(smem);
    const int ldf = R + 1;
#pragma unroll
    for (int i = 0; i < RT; ++i) {
        const int rt = wave + NW * i;
        if (rt >= n_rt) continue;
#pragma unroll
        for (int j = 0; j < PT; ++j) {
            const int px = j * 32 + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; ++r) df[(size_t)px * ldf + rt * 32 + acc_row(lane, r)] = acc[i][j][r];
        }
    }
    __syncthreads();
    if (dsk) {  // points_enc feeds layer 0 and every skip layer: its gradient is their sum
        for (int e = threadIdx.x; e < TP * R; e += 64 * NW) {
            const int px = e / R, c = e - px * R;
            df[(size_t)px * ldf + c] += dsk[e];
        }
        __syncthreads();
    }
    MARF_STAMP(sp, 17);

    // posenc adjoint: d coord_c = df[c] + sum_k w_k f_k (cos(x_k) df_sin - sin(x_k) df_cos)
    constexpr int NPART = 64 * NW / TP;
    const int i = threadIdx.x % TP, part = threadIdx.x / TP;
    float x, y, u = 0.f, v = 0.f, X[3] = {0.f, 0.f, 1.f};
    const bool valid = slot_point<GRID_ONLY>(geo, b, p0 + i, x, y, u, v, X);
    const float* row = df + (size_t)i * ldf;
    float du = 0.f, dv = 0.f;
    if (part == 0) {
        du += row[0];
        dv += row[1];
    }
    for (int q = part; q < 2 * L; q += NPART) {
        const int c = q >= L, k = q - c * L;
        float s, co;
        band_sincos<FAST>(c ? v : u, k, s, co);
        float gs = row[2 + q + c * L], gc = row[2 + q + c * L + L];
        if (c2f_on) {
            const float w = wsh[k];
            gs = gs * w;
            gc = gc * w;
        }
        float dspec = gs * co - gc * s;
        float d = dspec * ldexpf(3.14159265358979323846f, k);
        if (c == 0) du += d; else dv += d;
    }
    red[(part * TP + i) * 2] = du;
    red[(part * TP + i) * 2 + 1] = dv;
    __syncthreads();
    MARF_STAMP(sp, 18);
    float h9[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) h9[e] = 0.f;
    if ((int)threadIdx.x < TP) {
        du = red[i * 2];
        dv = red[i * 2 + 1];
        for (int q = 1; q < NPART; ++q) {
            du += red[(q * TP + i) * 2];
            dv += red[(q * TP + i) * 2 + 1];
        }
        if constexpr (UV_ONLY) {
            d_coords[2 * i] = du;
            d_coords[2 * i + 1] = dv;
        } else if (geo.mode == 1) {
            if (valid && d_coords) {
                d_coords[2 * (size_t)(p0 + i)] = du;
                d_coords[2 * (size_t)(p0 + i) + 1] = dv;
            }
        } else if (valid) {
            // (u, v) = X[:2] / (X[2] + 1e-8): torch div backward, then bmm backward
            float dd = X[2] + 1e-8f;
            float dX0 = du / dd, dX1 = dv / dd;
            float dd2 = dd * dd;
            float dX2 = (-du * X[0]) / dd2 + (-dv * X[1]) / dd2;
            const float hom[3] = {x, y, 1.f};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                h9[0 + c] = dX0 * hom[c];
                h9[3 + c] = dX1 * hom[c];
                h9[6 + c] = dX2 * hom[c];
            }
        }
    }
    if constexpr (UV_ONLY) return;
    if (geo.mode == 0) {
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            const float s = wave_total63(h9[e]);
            if (lane == 63) red9[wave * 9 + e] = s;
        }
        __syncthreads();
        if (threadIdx.x < 9) {
            float s = red9[threadIdx.x];
            for (int w = 1; w < NW; ++w) s += red9[w * 9 + threadIdx.x];
            dH_partial[(size_t)blockIdx.x * 9 + threadIdx.x] = s;
        }
    }
}

template <class P, int TP, bool GRID_ONLY = false, int NW = 4>
MARF_DEV void warp_adjoint(const NetDev& net, const GeoDev& geo, int c2f_on, const float* wsh, char* smem, int lda,
                           int wave, int lane, int b, int p0, float* red, float* red9, float* dH_partial,
                           float* d_coords, TileStore<typename P::T>& st, unsigned long long* sp = nullptr,
                           const float* dsk = nullptr) {
    typedef typename P::T T;
    constexpr int PT = TP / 32;
    constexpr int RT = 8 / PT;
    const T* act = reinterpret_cast<const T*>(smem);
    f32x16 acc[RT][PT];
    gemm_tile<P, RT, PT, NW>(acc, reinterpret_cast<const T*>(net.Wt[0]), net.Mt[0], net.Kp[0] / 32, act, lda, wave, lane,
                             nullptr, st);
    __syncthreads();
    MARF_STAMP(sp, 16);
    warp_adjoint_tail<P, TP, GRID_ONLY, NW, sizeof(T) == 2>(acc, net, geo, c2f_on, wsh, smem, wave, lane, b, p0, red, red9,
                                                           dH_partial, d_coords, sp, dsk);
}

// ======================================================================== all-operands-split bf16
//
// The mask network's MARF_BF16X3A recipe: every GEMM operand x is the pair hi = bf16_rne(x),
// lo = bf16_rne(x - float(hi)), and every product is hi*hi + hi*lo + lo*hi into one fp32 accumulator
// (lo*lo dropped).  Each operand lives in two planes of the same shape: the LDS tile [TP][lda] twice
// (lo at +TP*lda elements), the fragment-major weight image twice (lo at +rows*K elements).

// x0..x3 split into 4 hi and 4 lo bf16 (two packed RNE conversions per plane)
MARF_DEV void split4(float x0, float x1, float x2, float x3, uint2& hi, uint2& lo) {
    hi.x = PrecBF16::pk2(x0, x1);
    hi.y = PrecBF16::pk2(x2, x3);
    const float r0 = x0 - __uint_as_float(hi.x << 16), r1 = x1 - __uint_as_float(hi.x & 0xffff0000u);
    const float r2 = x2 - __uint_as_float(hi.y << 16), r3 = x3 - __uint_as_float(hi.y & 0xffff0000u);
    lo.x = PrecBF16::pk2(r0, r1);
    lo.y = PrecBF16::pk2(r2, r3);
}
MARF_DEV void split1(float x, u16& hi, u16& lo) {
    hi = f2bf(x);
    lo = f2bf(x - bf2f(hi));
}
MARF_DEV void store4_split(u16* dh, u16* dl, float x0, float x1, float x2, float x3) {
    uint2 hi, lo;
    split4(x0, x1, x2, x3, hi, lo);
    st_as<uint2>(dh, hi);
    st_as<uint2>(dl, lo);
}

// gemm_rows with both operands split: per k-step the A fragments hi + lo (the L2 register ring) and
// the B fragments hi + lo (LDS, two named buffers), 3 NA PT MFMAs into the same accumulators, the
// three terms outermost so NA PT independent MFMAs stand between two on one accumulator.  The issue
// order is pinned as in gemm_rows; the ring is 4 deep for NA <= 2, 2 deep above (register budget).
template <int NA, int RT, int PT, int NW = 4>
MARF_DEV void gemm_rows_split(f32x16 (&acc)[RT][PT], const u16* __restrict__ Wh, const u16* __restrict__ Wl, int K,
                              const u16* acth, const u16* actl, int lda, int wave, int lane, const float* bias) {
    typedef PrecBF16 P;
    typedef P::frag F;
    const int ko = P::kofs(lane);
    const int rl = lane & 31;
    const int nk = K / P::KS;
    // the accumulators start at the bias of their output row (set here, inside the NA dispatch: set
    // before it, the start values stayed live beside the accumulators through every case and spilled)
    if (bias) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const float* bb = bias + (wave + NW * i) * 32 + 4 * (lane >> 5);
            f32x16 init;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 bv = ld_as<float4>(bb + 8 * q);
                init[4 * q] = bv.x;
                init[4 * q + 1] = bv.y;
                init[4 * q + 2] = bv.z;
                init[4 * q + 3] = bv.w;
            }
#pragma unroll
            for (int j = 0; j < PT; ++j) acc[i][j] = init;
        }
    }
    size_t wofs[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) wofs[i] = ((size_t)(wave + NW * i) * nk * 64 + lane) * P::FE;
    const size_t bofs = (size_t)rl * lda + ko;
    auto ldA = [&](F (&dh)[NA], F (&dl)[NA], int k) {
        const int kc = (k < nk ? k : nk - 1) * 64 * P::FE;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            dh[i] = P::load_frag(Wh + wofs[i] + kc);
            dl[i] = P::load_frag(Wl + wofs[i] + kc);
        }
    };
    auto ldB = [&](F (&dh)[PT], F (&dl)[PT], int k) {
        const int kc = (k < nk ? k : nk - 1) * P::KS;
#pragma unroll
        for (int j = 0; j < PT; ++j) {
            dh[j] = P::load_frag(acth + bofs + (size_t)j * 32 * lda + kc);
            dl[j] = P::load_frag(actl + bofs + (size_t)j * 32 * lda + kc);
        }
    };
    auto mma = [&](const F (&ah)[NA], const F (&al)[NA], const F (&bh)[PT], const F (&bl)[PT]) {
#pragma unroll
        for (int j = 0; j < PT; ++j)
#pragma unroll
            for (int i = 0; i < NA; ++i) acc[i][j] = P::mma32(ah[i], bh[j], acc[i][j]);
#pragma unroll
        for (int j = 0; j < PT; ++j)
#pragma unroll
            for (int i = 0; i < NA; ++i) acc[i][j] = P::mma32(ah[i], bl[j], acc[i][j]);
#pragma unroll
        for (int j = 0; j < PT; ++j)
#pragma unroll
            for (int i = 0; i < NA; ++i) acc[i][j] = P::mma32(al[i], bh[j], acc[i][j]);
    };
    F A0h[NA], A0l[NA], A1h[NA], A1l[NA], B0h[PT], B0l[PT], B1h[PT], B1l[PT];
    if constexpr (NA > 2) {
        ldA(A0h, A0l, 0);
        ldA(A1h, A1l, 1);
        ldB(B0h, B0l, 0);
        int k = 0;
        for (; k + 2 <= nk; k += 2) {
            ldB(B1h, B1l, k + 1);
            __builtin_amdgcn_sched_barrier(0);
            mma(A0h, A0l, B0h, B0l);
            __builtin_amdgcn_sched_barrier(0);
            ldA(A0h, A0l, k + 2);
            ldB(B0h, B0l, k + 2);
            __builtin_amdgcn_sched_barrier(0);
            mma(A1h, A1l, B1h, B1l);
            __builtin_amdgcn_sched_barrier(0);
            ldA(A1h, A1l, k + 3);
        }
        if (k < nk) mma(A0h, A0l, B0h, B0l);
    } else {
        F A2h[NA], A2l[NA], A3h[NA], A3l[NA];
        ldA(A0h, A0l, 0);
        ldA(A1h, A1l, 1);
        ldA(A2h, A2l, 2);
        ldA(A3h, A3l, 3);
        ldB(B0h, B0l, 0);
        int k = 0;
        for (; k + 4 <= nk; k += 4) {
            ldB(B1h, B1l, k + 1);
            __builtin_amdgcn_sched_barrier(0);
            mma(A0h, A0l, B0h, B0l);
            __builtin_amdgcn_sched_barrier(0);
            ldA(A0h, A0l, k + 4);
            ldB(B0h, B0l, k + 2);
            __builtin_amdgcn_sched_barrier(0);
            mma(A1h, A1l, B1h, B1l);
            __builtin_amdgcn_sched_barrier(0);
            ldA(A1h, A1l, k + 5);
            ldB(B1h, B1l, k + 3);
            __builtin_amdgcn_sched_barrier(0);
            mma(A2h, A2l, B0h, B0l);
            __builtin_amdgcn_sched_barrier(0);
            ldA(A2h, A2l, k + 6);
            ldB(B0h, B0l, k + 4);
            __builtin_amdgcn_sched_barrier(0);
            mma(A3h, A3l, B1h, B1l);
            __builtin_amdgcn_sched_barrier(0);
            ldA(A3h, A3l, k + 7);
        }
        // remainder (nk % 4 steps): A0..A2 hold steps k..k+2, B0 holds step k
        if (k < nk) {
            ldB(B1h, B1l, k + 1);
            mma(A0h, A0l, B0h, B0l);
            if (k + 1 < nk) {
                ldB(B0h, B0l, k + 2);
                mma(A1h, A1l, B1h, B1l);
                if (k + 2 < nk) mma(A2h, A2l, B0h, B0l);
            }
        }
    }
}

// gemm_tile of the split recipe: the wave's row tiles dispatched once per layer, bias as the
// accumulators' start.  W: the hi image of rows x K elements, the lo image right behind it.  The saved
// tile's stores (two planes) go out after the GEMM, as in gemm_tile.
template <int RT, int PT, int NW = 4>
MARF_DEV void gemm_tile_split(f32x16 (&acc)[RT][PT], const u16* __restrict__ W, int rows, int K, const u16* acth,
                              const u16* actl, int lda, int wave, int lane, const float* bias, TileStore<u16>& sth,
                              TileStore<u16>& stl) {
    const int n_rt = rows / 32;
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < PT; ++j) acc[i][j] = (f32x16){};
    int na = (n_rt - wave + NW - 1) / NW;
    na = na < 0 ? 0 : (na > RT ? RT : na);
    const u16* Wl = W + (size_t)rows * K;
    switch (na) {
        case 1: gemm_rows_split<1, RT, PT, NW>(acc, W, Wl, K, acth, actl, lda, wave, lane, bias); break;
        case 2: gemm_rows_split<2, RT, PT, NW>(acc, W, Wl, K, acth, actl, lda, wave, lane, bias); break;
        case 3: if constexpr (RT >= 3) gemm_rows_split<3, RT, PT, NW>(acc, W, Wl, K, acth, actl, lda, wave, lane, bias); break;
        case 4: if constexpr (RT >= 4) gemm_rows_split<4, RT, PT, NW>(acc, W, Wl, K, acth, actl, lda, wave, lane, bias); break;
        default: break;
    }
    if (sth.active) sth.flush(acth);
    if (stl.active) stl.flush(actl);
}

// ======================================================================== tile views
//
// The rule of the tile kernels: a phase is written once, over a view of the LDS activation tile; a
// recipe is a view.
//   TileView<P>      one plane [TP][lda] of P::T (fp32, bf16, fp16)
//   SplitView<BOTH>  the all-operands-split recipe's two u16 planes, hi then lo.  BOTH is the save
//                    policy: false = a saved tile is its hi plane (k_mlp_step_split: plain bf16's
//                    bytes), true = both planes, the lo one S * cols elements behind the hi one (the
//                    mask kernels; S = all pixel slots)
// Both offer: row (a slot's row, + column = an element: Ref), put / put4 / zero (element stores: one
// conversion, or the split into both planes),
// gemm (the layer GEMM into the wave's accumulators; it flushes the queued save), w16 / mma16_row
// (one k-step of the 16-row last layer: one term, or the recipe's three), queue_save / flush /
// clear_save over the TileStore(s), save_last_input (the tile as the last-layer weight gradient
// reads it) and feat() (the plane the fused last-layer weight gradient reads).  Structs of pointers:
// every member inlines, nothing is dispatched at run time.  The phase functions take a view by value:
// taken by reference, k_mlp_step's register allocation moved (4 - 8 B more scratch in its skip
// instantiations, profiles/tile_view/README.md); by value every kernel keeps the parent's.
template <class P_>
struct TileView {
    typedef P_ P;
    typedef typename P::T T;
    typedef typename P::frag W16;  // the last layer's weight fragment of one k-step
    static constexpr bool SPLIT = false;
    T* act;
    int lda;
    TileStore<T> st;

    MARF_DEV TileView(char* smem, int lda_, int /*TP*/) : act(reinterpret_cast<T*>(smem)), lda(lda_) { st.clear(); }
    typedef T* Ref;  // an element of the tile: row(px) + column
    MARF_DEV Ref row(int px) const { return act + (size_t)px * lda; }
    MARF_DEV const T* feat() const { return act; }
    MARF_DEV void put(Ref at, float x) const { *at = P::cvt(x); }
    MARF_DEV void put4(Ref at, float x0, float x1, float x2, float x3) const { store4<P>(at, x0, x1, x2, x3); }
    MARF_DEV void zero(Ref at) const { *at = P::cvt(0.f); }
    // W: rows x K, fragment-major
    template <int RT, int PT, int NW>
    MARF_DEV void gemm(f32x16 (&acc)[RT][PT], const void* W, int rows, int K, const float* bias, int wave, int lane) {
        gemm_tile<P, RT, PT, NW>(acc, reinterpret_cast<const T*>(W), K, rows / 32, act, lda, wave, lane, bias, st);
    }
    MARF_DEV static W16 w16(const void* W, int /*K*/, int u, int lane) {
        return P::load_frag(reinterpret_cast<const T*>(W) + ((size_t)u * 64 + lane) * P::FE);
    }
    MARF_DEV f32x4 mma16_row(const W16& w, int px, int u, int lane, f32x4 acc) const {
        return P::mma16(w, P::load_frag(act + (size_t)px * lda + u * P::KS16 + P::kofs16(lane)), acc);
    }
    // the tile's first `cols` columns -> rows slot0 .. of dst [S][cols]: 16-bit tiles stream out
    // behind the next gemm, fp32 tiles are copied right away (save_tile)
    template <int NW>
    MARF_DEV void queue_save(void* dst, long long slot0, long long /*S*/, int rows, int cols, int rmode = 0) {
        save_tile<P, NW>(st, act, lda, rows, cols, reinterpret_cast<T*>(dst) + slot0 * cols, rmode);
    }
    MARF_DEV void flush() {
        if (st.active) st.flush(act);
    }
    MARF_DEV void clear_save() { st.clear(); }
    MARF_DEV void save_last_input(void* dst, long long slot0, int rows, int cols) const {  // plain copy
        copy_tile_out<P>(act, lda, rows, cols, reinterpret_cast<T*>(dst) + slot0 * cols, cols);
    }
};

template <bool BOTH>
struct SplitView {
    typedef PrecBF16 P;
    typedef u16 T;
    struct W16 {
        P::frag hi, lo;
    };
    static constexpr bool SPLIT = true;
    u16 *hi, *lo;
    int lda;
    TileStore<u16> sth, stl;

    MARF_DEV SplitView(char* smem, int lda_, int TP) : hi(reinterpret_cast<u16*>(smem)), lo(hi + (size_t)TP * lda_), lda(lda_) {
        sth.clear();
        stl.clear();
    }
    typedef size_t Ref;  // the element's offset in either plane
    MARF_DEV Ref row(int px) const { return (size_t)px * lda; }
    MARF_DEV const u16* feat() const { return hi; }
    MARF_DEV void put(Ref at, float x) const { split1(x, hi[at], lo[at]); }
    MARF_DEV void put4(Ref at, float x0, float x1, float x2, float x3) const {
        store4_split(hi + at, lo + at, x0, x1, x2, x3);
    }
    MARF_DEV void zero(Ref at) const {
        hi[at] = 0;
        lo[at] = 0;
    }
    // W: the hi image of rows x K elements, the lo image right behind it
    template <int RT, int PT, int NW>
    MARF_DEV void gemm(f32x16 (&acc)[RT][PT], const void* W, int rows, int K, const float* bias, int wave, int lane) {
        gemm_tile_split<RT, PT, NW>(acc, reinterpret_cast<const u16*>(W), rows, K, hi, lo, lda, wave, lane, bias, sth, stl);
    }
    MARF_DEV static W16 w16(const void* W, int K, int u, int lane) {  // 16 padded rows: lo image at + 16 K
        const u16* Wh = reinterpret_cast<const u16*>(W);
        const u16* Wl = Wh + (size_t)16 * K;
        const size_t wo = ((size_t)u * 64 + lane) * P::FE;
        const P::frag wh = P::load_frag(Wh + wo), wl = P::load_frag(Wl + wo);
        return W16{wh, wl};
    }
    MARF_DEV f32x4 mma16_row(const W16& w, int px, int u, int lane, f32x4 acc) const {  // the same three terms
        const size_t bo = (size_t)px * lda + u * P::KS16 + P::kofs16(lane);
        const P::frag bh = P::load_frag(hi + bo), bl = P::load_frag(lo + bo);
        acc = P::mma16(w.hi, bh, acc);
        acc = P::mma16(w.hi, bl, acc);
        return P::mma16(w.lo, bh, acc);
    }
    template <int NW>
    MARF_DEV void queue_save(void* dst, long long slot0, long long S, int rows, int cols, int = 0) {
        const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        u16* d = reinterpret_cast<u16*>(dst);
        sth.init(lda, d + slot0 * cols, cols, rows, cols, wave, lane, NW);
        if constexpr (BOTH) stl.init(lda, d + (S + slot0) * cols, cols, rows, cols, wave, lane, NW);
    }
    MARF_DEV void flush() {
        if (sth.active) sth.flush(hi);
        if (stl.active) stl.flush(lo);
    }
    MARF_DEV void clear_save() {
        sth.clear();
        stl.clear();
    }
    // fp32 [S][cols] = float(hi) + float(lo): what the fp32 last-layer weight gradient reads
    MARF_DEV void save_last_input(void* dst, long long slot0, int rows, int cols) const {
        float* d = reinterpret_cast<float*>(dst) + slot0 * cols;
        for (int e = threadIdx.x; e < rows * cols; e += blockDim.x) {
            const int r = e / cols, c = e - r * cols;
            d[(size_t)r * cols + c] = bf2f(hi[(size_t)r * lda + c]) + bf2f(lo[(size_t)r * lda + c]);
        }
    }
};

// Hidden-layer epilogue: ReLU of the accumulators (bias already in them) written back to the tile in
// place, and (mk != null) the ReLU mask record of this wave.  Per element: v_cmp (vcc = z > 0),
// v_cndmask (relu), v_addc (shift the bit into the tile's mask word).
template <int RT, int PT, int NW = 4, class V>
MARF_DEV void relu_epilogue(f32x16 (&acc)[RT][PT], V v, int n_rt, int wave, int lane, uint64_t* mk, int tile,
                            unsigned diag_next = 0) {
    static_assert(RT * PT <= 8, "a wave's ReLU mask record holds 8 accumulator tiles of 16 bits");
    (void)diag_next;  // (the next layer's rounding code: MARF_DIAG_RT builds, plain views only)
    uint32_t words[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < RT; ++i) {
        const int rt = wave + NW * i;
        if (rt >= n_rt) continue;
        const int rbase = rt * 32 + 4 * (lane >> 5);
#pragma unroll
        for (int j = 0; j < PT; ++j) {
            const int ti = i * PT + j;
            const int px = j * 32 + (lane & 31);
            float o[16];
            uint32_t bits = 0;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float x;
                asm volatile(
                    "v_cmp_lt_f32_e32 vcc, 0, %2\n\t"
                    "v_cndmask_b32_e32 %0, 0, %2, vcc\n\t"
                    "v_addc_co_u32_e32 %1, vcc, %1, %1, vcc"
                    : "=&v"(x), "+v"(bits)
                    : "v"(acc[i][j][r])
                    : "vcc");
                o[r] = x;
                if constexpr (!V::SPLIT) o[r] = MARF_DIAG_ROUND(o[r], diag_next, 2);
            }
            words[ti >> 1] |= bits << (16 * (1 - (ti & 1)));
#pragma unroll
            for (int q = 0; q < 4; ++q) v.put4(v.row(px) + rbase + 8 * q, o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
        }
    }
    if (mk) *mask_record(mk, tile, wave, lane, NW) = make_uint4(words[0], words[1], words[2], words[3]);
}

// Dgrad epilogue: dz = acc * relu'(feat) with this wave's mask record `mw` (loaded before the GEMM),
// written to the tile.  Per element: v_bfe_i32 (0 / -1 from the bit) and v_and.
template <int RT, int PT, int NW = 4, class V>
MARF_DEV void mask_epilogue(f32x16 (&acc)[RT][PT], V v, int n_rt, int wave, int lane, uint4 mw,
                            unsigned diag_out = 0) {
    static_assert(RT * PT <= 8, "a wave's ReLU mask record holds 8 accumulator tiles of 16 bits");
    (void)diag_out;  // (the rounding code of the layer whose output gradient this is: MARF_DIAG_RT)
    const uint32_t words[4] = {mw.x, mw.y, mw.z, mw.w};
#pragma unroll
    for (int i = 0; i < RT; ++i) {
        const int rt = wave + NW * i;
        if (rt >= n_rt) continue;
        const int rbase = rt * 32 + 4 * (lane >> 5);
#pragma unroll
        for (int j = 0; j < PT; ++j) {
            const int ti = i * PT + j;
            const int px = j * 32 + (lane & 31);
            const uint32_t w = words[ti >> 1];
            float o[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = __builtin_amdgcn_sbfe((int)w, 16 * (1 - (ti & 1)) + 15 - r, 1);
                o[r] = __int_as_float(__float_as_int(acc[i][j][r]) & m);
                if constexpr (!V::SPLIT) o[r] = MARF_DIAG_ROUND(o[r], diag_out, 3);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) v.put4(v.row(px) + rbase + 8 * q, o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
        }
    }
}

// One dgrad layer of the plain tile kernels: dz_l = (W_l^T dz_{l+1}) * relu'(feat_l) into the tile (the
// ReLU record of feat_l), and for a skip layer the posenc rows into dsk.  acc holds the GEMM.
template <int RT, int PT, int NW = 4, class V>
MARF_DEV void dgrad_epilogue(f32x16 (&acc)[RT][PT], const NetDev& net, int l, V v, int wave, int lane, uint4 mw,
                             float* dsk) {
    const int R = net.Kp[l];
    if (dsk && ((net.skip >> l) & 1u)) {  // (dsk: null in kernels built without skip support)
        mask_epilogue<RT, PT, NW>(acc, v, net.Mp[l - 1] / 32, wave, lane, mw, net.diag[l - 1]);
        skip_epilogue<typename V::P, RT, PT, NW>(acc, dsk, net.Kp[0], net.Mp[l - 1] / 32, R / 32, wave, lane);
    } else {
        mask_epilogue<RT, PT, NW>(acc, v, R / 32, wave, lane, mw, net.diag[l - 1]);
    }
}

// ======================================================================== last layer, forward
//
// NOUT <= 3 real output rows (padded to 16) in the 16x16 MFMA form: a wave takes TP / NW pixels in
// NJ = TP / NW / 16 groups of 16; acc[j][c] is row c of pixel wave * (TP / NW) + j * 16 + lane, held
// in lanes 0 - 15.
template <int TP, int NW, class V>
MARF_DEV void last_layer_gemm(V v, const void* W, int K, int wave, int lane, f32x4 (&acc)[TP / NW / 16]) {
    constexpr int NJ = TP / NW / 16;
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = (f32x4){};
    // (the loop runs on k0 and w16 names both weight loads: counted in k-steps, with the lo image's
    // address formed in the load, the split view's lo weight load sank behind the two hi MFMAs -- two
    // serial L2 latencies per k-step, and the C5 step and render about 1 % and 1.6 % slower)
    for (int k0 = 0; k0 < K; k0 += V::P::KS16) {
        const typename V::W16 w = V::w16(W, K, k0 / V::P::KS16, lane);
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            acc[j] = v.mma16_row(w, wave * (TP / NW) + j * 16 + (lane & 15), k0 / V::P::KS16, lane, acc[j]);
    }
}

// ... then bias and sigmoid (fp32) of the tile's real pixels to out_all[b][p][NOUT]
template <int TP, int NW, int NOUT, class V>
MARF_DEV void last_layer_fwd(V v, const NetDev& net, int wave, int lane, int b, int p0, int Np, float* out_all) {
    constexpr int NJ = TP / NW / 16;
    const int l = net.n_layers - 1;
    f32x4 acc[NJ];
    last_layer_gemm<TP, NW>(v, net.Wf[l], net.Kp[l], wave, lane, acc);
    if (lane < 16) {
        const float* bias = net.bias[l];
        float* out = out_all + (size_t)b * Np * NOUT;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int p = p0 + wave * (TP / NW) + j * 16 + lane;
            if (p < Np) {
                float* o = out + (size_t)p * NOUT;
#pragma unroll
                for (int c = 0; c < NOUT; ++c) {
                    const float z = acc[j][c] + bias[c];
                    o[c] = 1.0f / (1.0f + expf(-z));
                }
            }
        }
    }
}

// ======================================================================== loss tail of the fused step
//
// Shared by k_mlp_step and k_mlp_step_split.  gl / gT / lsum are the kernel's own __shared__ arrays,
// taken by reference to array so every access stays an LDS access.

// Target + mask of the tile's slots, loaded at the kernel's start and parked in gl until the loss
// needs them.  Straight-line (every thread loads, padding slots a clamped valid pixel, zeroed after)
// so the compiler counts the loads and an early barrier need not wait for them.
template <int TP>
MARF_DEV float4 step_target(const StepArgs& a, int b, int p0) {
    const int Np = a.geo.Np;
    const int ti = threadIdx.x & (TP - 1);
    const int pc = min(p0 + ti, Np - 1);
    const float* gb = a.gt + (size_t)b * 3 * Np + pc;
    const float* mb = a.mask ? a.mask + (size_t)b * Np + pc : gb;
    float4 tg = make_float4(gb[0], gb[Np], gb[2 * (size_t)Np], mb[0]);
    if (!a.mask) tg.w = 1.0f;
    if (p0 + ti >= Np) tg = make_float4(0.f, 0.f, 0.f, 0.f);
    return tg;
}

// Per slot of the wave's 16-pixel groups (lanes 0 - 15; acc = last_layer_gemm's): sigmoid, rgb,
// masked-MSE partial and d rgb, sigmoid backward -> gl (fp32), gT (channel-major, hi + lo of P::T),
// lsum (((p-g) m)^2 and m).
template <class P, int TP, int NW, int NJ>
MARF_DEV void step_loss_slots(const StepArgs& a, const f32x4 (&acc)[NJ], int wave, int lane, int b, int p0,
                              float (&gl)[TP][4], typename P::T (&gT)[8][TP], float (&lsum)[2][TP]) {
    typedef typename P::T T;
    const int Np = a.geo.Np;
    if (lane < 16) {
        const float* bl = a.net.bias[a.net.n_layers - 1];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int px = wave * (TP / NW) + j * 16 + lane;
            const int p = p0 + px;
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
            for (int c = 0; c < 3; ++c) {  // g = hi + lo (bf16 pair: ~16 significant bits)
                const T hi = P::cvt(g[c]);
                gT[c][px] = hi;
                gT[4 + c][px] = P::cvt(g[c] - P::tof(hi));
            }
            gT[3][px] = P::cvt(0.f);
            gT[7][px] = P::cvt(0.f);
            lsum[0][px] = sq;
            lsum[1][px] = mv;
        }
    }
}

// Masked-MSE partial of the tile (fp64, fixed order; wave 0) and the last bias gradient (wave 1;
// BLAST = false: the warp-only step has no bias gradient).
template <int TP, bool BLAST = true>
MARF_DEV void step_tile_partials(const StepArgs& a, int wave, int lane, const float (&gl)[TP][4],
                                 const float (&lsum)[2][TP]) {
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
    } else if (BLAST && wave == 1) {
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
}

// Last-layer weight gradient of the tile: dW[c][k] = sum_px g[px][c] feat[px][k] (feat: the tile
// plane [TP][lda] holding feat_{n-1}; a split view's hi plane).  16x16 MFMA, A = g^T (rows 0-2: the
// hi parts of the 3 channels, rows 4-6: lo parts), B = feat (pixels x features, transposed LDS read
// for 16-bit T); hi + lo rows are added after the K loop.  Column tiles of 16 features dealt
// round-robin to the waves.
template <class P, int TP, int NW>
MARF_DEV void step_wlast_grad(const StepArgs& a, int Kl, const typename P::T* feat, int lda, int wave, int lane,
                              const typename P::T (&gT)[8][TP]) {
    typedef typename P::T T;
    float* wout = a.wlast_partial + (size_t)blockIdx.x * 3 * Kl;
    for (int ct = wave; ct < Kl / 16; ct += NW) {
        f32x4 acc = (f32x4){};
        if constexpr (sizeof(T) == 2) {
            const int g = lane >> 4, gi = lane & 15;
#pragma unroll
            for (int k0 = 0; k0 < TP; k0 += 32) {
                typename P::frag fa;
                if (gi < 8) fa = P::load_frag(&gT[gi][k0 + 8 * g]);
                else fa = (typename P::frag){};
                const int r0 = k0 + 8 * g + (gi >> 2);
                const u16* base = feat + (size_t)r0 * lda + ct * 16 + 4 * (gi & 3);
                acc = P::mma16(fa, frag_of<typename P::frag>(tr_read16(base), tr_read16(base + 4 * lda)), acc);
            }
        } else {
            const int kk = lane >> 4, n = lane & 15;
            for (int k0 = 0; k0 < TP; k0 += 4) {
                const float fa = n < 8 ? P::tof(gT[n][k0 + kk]) : 0.f;
                const float fb = P::tof(feat[(size_t)(k0 + kk) * lda + ct * 16 + n]);
                acc = P::mma16(fa, fb, acc);
            }
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

// d (last-layer input) operand of the dgrad chain: tile columns 0 .. Kt) of every slot = g (gl), zero
// past the 3 channels.  (A split view stores split1(g): the bits of gT's hi and lo rows.)
template <int TP, class V>
MARF_DEV void step_fill_d(V v, const float (&gl)[TP][4], int Kt, unsigned diag) {
    (void)diag;  // (MARF_DIAG_RT builds, plain views only)
    if ((int)threadIdx.x < TP) {
        const int i = threadIdx.x;
        for (int c = 0; c < Kt; ++c) {
            float x = c < 3 ? gl[i][c] : 0.f;
            if constexpr (!V::SPLIT) x = MARF_DIAG_ROUND(x, diag, 3);
            v.put(v.row(i) + c, x);
        }
    }
}

}  // namespace marf
