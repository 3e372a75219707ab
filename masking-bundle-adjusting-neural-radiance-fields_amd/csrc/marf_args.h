// marf_args.h -- kernel argument blocks and host launcher prototypes shared by the .hip units.
#pragma once
#include "marf_common.h"

namespace marf {

struct C2fDev {
    const float* progress;  // device scalar (NeuralImageFunction.progress)
    float start, span;      // barf_c2f start, end - start
    int on;
};

struct FwdArgs {
    NetDev net;
    GeoDev geo;
    C2fDev c2f;
    float* rgb;                       // [B][Np][3]
    void* feat[MARF_MAX_LAYERS];      // saved layer inputs [S][Kp_l] (nullptr: do not save)
    uint64_t* mask[MARF_MAX_LAYERS];  // relu masks of feat_l (l >= 1), wave-ballot layout (marf_common.h)
    long long S;
    int lda;                          // LDS row stride (elements)
};

struct BwdArgs {
    NetDev net;
    GeoDev geo;
    C2fDev c2f;
    const float* rgb;                       // [B][Np][3] forward output
    const float* d_rgb;                     // [B][Np][3]
    const uint64_t* mask[MARF_MAX_LAYERS];  // from forward
    void* dz[MARF_MAX_LAYERS];              // out: dz_l (l >= 1) [S][Kp_l] (grad of layer l-1 pre-act)
    float* glast;                           // out: [S][4] grad of the last layer pre-activation
    float* dH_partial;                      // out (geo mode 0): [n_tiles][9]
    float* d_coords;                        // out (geo mode 1): [Np][2] (may be null)
    long long S;
    int lda;
};

// Fused training step of the grid geometry (marf_step.hip): forward, masked MSE with unit upstream
// gradient, dgrad chain and warp adjoint in one pass over each tile.
struct StepArgs {
    NetDev net;
    GeoDev geo;
    C2fDev c2f;
    float* rgb;                             // [B][Np][3] forward output (may be null)
    const float* gt;                        // [B][3][Np] target
    const float* mask;                      // [B][1][Np] or null (plain mean)
    void* feat[MARF_MAX_LAYERS];            // out: inputs of layers 0 .. n-2 [S][Kp_l]
    uint64_t* mask_bits[MARF_MAX_LAYERS];   // scratch: ReLU masks of feat_l, l = 1 .. n-1
    void* dz[MARF_MAX_LAYERS];              // out: dz_l, l = 1 .. n-1 [S][Kp_l]
    float* wlast_partial;                   // out: [n_tiles][3][Kp_{n-1}] last-layer weight gradient
    float* blast_partial;                   // out: [n_tiles][3]
    float* dH_partial;                      // out: [n_tiles][9]
    double* loss_partial;                   // out: [n_tiles][2] = sum ((p - g) m)^2, sum m
    const float* c2f_w;                     // [L] band weights of this step (k_c2f_weights)
    unsigned long long* stamps;             // diagnostic builds (MARF_STAMPS): [n_tiles][32] s_memtime
    long long S;
    int lda;
};

// Gauss-Newton normal equations on a frozen image (marf_gn.hip): the step's inputs (s: net, geo, c2f,
// rgb, gt, mask, mask_bits, c2f_w, lda; nothing is saved, no dH / loss partials) and the per-tile
// partials [n_tiles][56] = sse, msum, g9 (9), N upper triangle row-major (45).  The robust
// instantiations (marf_gn_normal_robust) read the last three: the loss (MARF_GN_HUBER / MARF_GN_CAUCHY),
// its scale and the per-pixel weight map; the others never look at them.
constexpr int GN_HUBER = 1, GN_CAUCHY = 2;  // include/marf.h's MARF_GN_HUBER / MARF_GN_CAUCHY
struct GnArgs {
    StepArgs s;
    double* partial;
    int robust_kind;
    float robust_delta;
    float* weight;  // out: [B][Np] IRLS weight of every real pixel (may be null)
};

// Implicit-mask network (marf_mask.hip; reference model/planar.py:340-349, 475-488): the per-pixel
// input [E[r] ; E[g] ; E[b] ; uv] is built in LDS, the layers run as the tile kernels' do.
struct MaskFwdArgs {
    NetDev net;                       // D = 3 * embed_dim + 2 + 4 * n_freqs, Kp[0] = D padded to 32
    GeoDev geo;                       // crop grid (Hm unused: the mask net sees the unwarped grid)
    const float* embed;               // [n_vocab][embed_dim] (embedding_view.weight)
    const int* index;                 // [B][3][Np] vocabulary rows of the three channels
    int n_vocab, embed_dim, n_freqs;
    float* m;                         // out: [B][1][Np] sigmoid output
    void* feat[MARF_MAX_LAYERS];      // saved layer inputs [S][Kp_l] (null: inference)
    uint64_t* mask[MARF_MAX_LAYERS];  // ReLU mask records of feat_l, l >= 1
    int lda;
    int split;                        // MARF_BF16X3A: two bf16 planes (hi, lo) per operand and saved tensor
};

struct MaskBwdArgs {
    NetDev net;
    GeoDev geo;
    const float* m;                         // [B][1][Np] forward output
    const float* dm;                        // [B][1][Np] upstream gradient
    const uint64_t* mask[MARF_MAX_LAYERS];  // from the forward
    void* dz[MARF_MAX_LAYERS];              // out: dz_l, l = 1 .. n-1 [S][Kp_l]
    float* glast;                           // out: [S][4], rows 1..3 zero
    int lda;
    int split;                              // MARF_BF16X3A (dz_l: hi plane [S][Kp_l], then the lo plane)
};

struct PackLayer {
    int M, K;                            // true dims (nn.Linear weight [M][K])
    int Mp, Kp, Mt;                      // padded: Wf [Mp][Kp], Wt [Kp][Mt], bias [Mp]
    long long w_off, b_off;              // offsets in the flat fp32 parameter vector
    long long wf_off, wt_off, bias_off;  // byte offsets in the packed buffer
    unsigned diag;                       // numerics-experiment rounding code (marf_common.h)
};

struct PackArgs {
    int n_layers;
    PackLayer ly[MARF_MAX_LAYERS];
};

// ---- dz_{n-1} recomputed by the weight gradient of layer n-2.  Instead of the
// 512 B / pixel of dz_{n-1} the step kernel stores what determines it, per 32-pixel set (= one
// wave's pixels = 32 consecutive pixel slots):
//   g    [S / 32 + NW][32][16 B]   the last-layer dgrad's B fragment of lane half 0 (pixel p:
//                                  [g hi (3), 0, g lo (3), 0] bf16; lane half 1 holds zeros)
//   mk   [S / 32 + NW][64][4]      the ReLU mask words of layer n-2's output: lane-major, word j =
//                                  row tiles 2 j, 2 j + 1
// and block 0 copies the 8 row tiles of the last-layer dgrad stage of the weight program, hi then lo
// (1 KB each), into w.  (The NW sets past S: the sink of a dgrad pass's set without a tile.)
constexpr int DZL_G_SET = 512, DZL_MK_SET = 1024, DZL_W_BYTES = 16384;

// Per-layer constants, copied into LDS at kernel start (kept out of the SGPR file).
struct S2Layer {
    int nrt;     // row tiles of the forward output (Mp / 32; last layer: 1)
    int nrtb;    // row tiles of the dgrad output (Kp / 32; layer 0: the adjoint tiles)
    int boff;    // offset of the padded bias in the bias table
    int ldf;     // row stride of feat_l (elements)
    int ldz;     // row stride of dz_l
    int pad;
    u16* feat;   // feat_l [S][ldf] bf16 (l = 0 .. nl-2)
    u16* dz;     // dz_l [S][ldz] bf16 (l = 1 .. nl-1)
};

struct Step2Args {
    GeoDev geo;                      // Np_pad is a multiple of 32 * NW
    int nl, L, nk0, nta, c2f_on;
    int r0;                          // layer-0 row tiles per stage
    const char* prog;                // weight stage program: n_stages slots of SLOT bytes
    int n_stages;
    int n_fwd;                       // the program's forward stages (the first n_fwd; the rest: dgrad)
    long long S;                     // pixel slots; rows S .. S + 32 NW - 1 of dz_l / dH: store sink
                                     // of a backward pixel set that has no tile (odd tile count)
    const float* bias;               // padded biases
    int nbias;                       // floats in the bias table
    const float* gt;                 // [B][3][Np]
    const float* mask;               // [B][1][Np] or null
    float* rgb;                      // [B][Np][3] or null
    S2Layer layers[MARF_MAX_LAYERS]; // per-layer table (copied into LDS at kernel start)
    float* dH_partial;               // [S / 32 + NW][9]
    double* loss_partial;            // [grid][2]
    float* blast_partial;            // [grid][3]
    float* wlast_partial;            // [grid][3][Kl]
    int Kl;                          // padded input width of the last layer
    const float* c2f_w;              // [L] band weights of this step
    float* dummy;                    // [grid][NW][ST][64][2] store sink
    unsigned long long* stamps;      // diagnostic builds (MARF_STAMPS): [grid][8] cycle totals of wave 0
    int tile0, n_tiles;              // this launch's block tiles [tile0, n_tiles) of 32 * NW pixel slots
    int fwd_only;                    // render: forward stages only, rgb out, nothing saved
    int feat0_recompute;             // feat_0 is recomputed by the layer-0 weight gradient: not stored
    const float* pro_fallback;       // valid device address for the input DMA when gt / H are absent
    // dz_{n-1} is recomputed by the weight gradient of layer n-2 (all null: stored as every dz_l): the
    // per-set g fragments, mask words and the dgrad stage's weights it needs (DZL_G_SET .. above)
    char* dzl_g;
    char* dzl_mk;
    char* dzl_w;
    // LDS layout (byte offsets; computed on the host)
    int lds_pro, lds_bias, lds_c2f, lds_layers, lds_wave, lds_wave_bytes, lds_total;
};

struct Pack2Args {
    int nl, L, nk0, nta, NKH, split, slot_bytes, n_stages;
    int fwd_f16;                     // forward stages in fp16 hi + lo (the fp16x2 recipe)
    int r0, ns0;                     // layer-0 row tiles per stage, layer-0 stages
    int dims[MARF_MAX_LAYERS + 1];   // true widths
    int nrt[MARF_MAX_LAYERS], nrtb[MARF_MAX_LAYERS];
    long long w_off[MARF_MAX_LAYERS], b_off[MARF_MAX_LAYERS];  // flat parameter offsets
    int boff[MARF_MAX_LAYERS];       // padded bias table offsets
    int Mp[MARF_MAX_LAYERS];
    int nbias;
};

// Raise a kernel's dynamic-LDS limit to at least `lds` bytes before a launch.  The limit set so
// far is tracked per (device, kernel) under a mutex, so a later launch of the same instantiation
// with a larger tile (a wider net) raises it again, and concurrent host threads do not race.
hipError_t ensure_dynamic_lds(const void* kernel, size_t lds);

}  // namespace marf

hipError_t marf_launch_sl3(const float* h, float* H, int B, int batch_hint, hipStream_t s);
hipError_t marf_launch_se2_embed(const float* p, float* h, int B, hipStream_t s);
hipError_t marf_launch_se2_embed_bwd(const float* dh, float* dp, int B, hipStream_t s);
hipError_t marf_launch_sl3_bwd(const float* h, const float* dH, float* dh, int B, int batch_hint, hipStream_t s);
hipError_t marf_launch_reduce_dH(const float* partial, int tiles_per_patch, int B, const float* h, float* dH_out,
                                 float* dh, int batch_hint, hipStream_t s, const float* gscale = nullptr,
                                 const float* denom = nullptr);
hipError_t marf_launch_mlp_fwd(const marf::FwdArgs& a, int dtype, int TP, size_t lds, int n_tiles, hipStream_t s);
hipError_t marf_launch_mlp_bwd(const marf::BwdArgs& a, int dtype, int TP, size_t lds, int n_tiles, hipStream_t s);
// ---- weight gradients (marf_wgrad.hip): dW_l = sum_px dz_{l+1} (x) feat_l as split-K partials
// [n_chunks][M][K] (+ [n_chunks][M] for the bias), then a fixed-order reduction.  A gradient is
// described once, as a WgJob: its shape (all that decides the kernel, known when the buffers are
// planned) and its pointers.  wg_pick holds every kernel's shape conditions: the plans ask it what
// a launch will do, marf_launch_wgrad does what it says.

// one piece of a pipelined step's weight gradients: n blocks split the pixel rows [s_lo, s_lo + s_len)
// and write split-K partials part0 .. part0 + n - 1
struct WgRange {
    long long s_lo, s_len;
    int n, part0;
};
// dz_{n-1} recomputed by the weight gradient of layer n-2 instead of read: what the step kernel
// stored in its place (DZL_G_SET .. above: per-set g fragments and mask words, the dgrad stage's weights)
struct WgDzlSrc {
    const char* g;
    const char* mk;
    const char* w;
};
struct WgShape {
    int dtype;            // 0 fp32, 1 bf16, 2 fp16
    int M, ldz, K, ldf;   // output rows (<= ldz) and columns (<= ldf); the operands' row strides
    long long S;          // pixel rows
    int chunk, n_chunks;  // the split-K rule (range mode: chunk unused, n_chunks = the range's blocks)
    bool t16;             // dz / feat in the split-recipe step kernel's T16 block layout (marf_wgrad.hip t16_off)
    bool split;           // MARF_BF16X3A (the mask net): each operand as bf16 hi + lo planes,
                          // dW = dz_h^T a_h + dz_h^T a_l + dz_l^T a_h, db = sum (dz_h + dz_l)
    bool f0;              // layer 0 with feat_0 recomputed on chip, not read (K = ldf: the step kernel's ldf0)
    bool dzl;             // layer n-2 with dz_{n-1} recomputed, not read (WgDzlSrc)
    bool ranged;          // range mode (WgRange)
    int L;                // f0: the net's posenc bands
    long long Np_pad;     // f0: pixel slots per patch
};
struct WgJob : WgShape {
    const void* dz;       // [S][ldz] (split: the hi plane)
    const void* dz_lo;    // split only
    const void* feat;     // [S][ldf] (split: the hi plane; f0: unused)
    const void* feat_lo;  // split only
    float* partial;       // [n_chunks][M][K]
    float* bpartial;      // [n_chunks][M], may be null
    WgDzlSrc dzl_src;     // dzl
    const GeoDev* f0_geo; // f0: the step's crop grid, its band weights (null: c2f off) and feat_0's
    const float* c2f_w;   //     column layout (k_step2's layer-0 k-steps)
    int nk0;
    WgRange rng;          // ranged
};
enum WgKernel { WG_NONE, WG_STAGED, WG_STAGED_SPLIT, WG_DMA256, WG_DMA96, WG_DMA_F0, WG_DMA_DZL };
struct WgPick {
    WgKernel k;
    int bm, bn;  // its output block (WG_STAGED: 256 x 256, 256 x 128, 256 x 64 or 128 x 64)
    constexpr int blocks(const WgShape& w) const { return ((w.M + bm - 1) / bm) * ((w.K + bn - 1) / bn); }
};
constexpr int WG_SPH = 32, WG_SP0 = 64;  // LDS-DMA stage heights: hidden layers, recomputed layer 0
constexpr int F0_PATCHES = 4;            // patches a recomputed layer-0 chunk may span
constexpr int WG_RANGE_CHUNK = 64;       // range mode's chunk: a multiple of every stage height it splits at

// The kernel an M x K weight gradient runs on, WG_NONE if there is none (a launch of it is an error).
constexpr WgPick wg_pick(const WgShape& w, bool dma_enabled) {
    constexpr WgPick none = {WG_NONE, 0, 0};
    const int chunk = w.ranged ? WG_RANGE_CHUNK : w.chunk;
    if (w.split)  // register-staged, 32-pixel stages; the mask net's layer 0 (K = 448) takes two column blocks
        return w.dtype == 1 && !w.t16 && !w.f0 && !w.dzl && !w.ranged && w.ldz % 8 == 0 && w.ldf % 8 == 0 &&
                       chunk % 32 == 0 && w.n_chunks >= 1
                   ? WgPick{WG_STAGED_SPLIT, 256, 256}
                   : none;
    // feat_0 recomputed: 256-wide layer 0, the 64-wide feat_0 of L <= 12 or the 96-wide one of
    // L = 13..16 (both built in the 96-wide stage; a 64-wide partial takes its first 64 columns).
    // L <= 16: the stage's 16 threads per row build two bands of one coordinate each, so bands
    // 16..19 of L = 17..20 (feat_0 96 wide too) would stay unwritten; those nets store and read feat_0
    if (w.f0)
        return w.dtype != 0 && !w.dzl && w.M == 256 && w.ldz % 8 == 0 && w.ldz >= w.M && (w.ldf == 96 || w.ldf == 64) &&
                       w.K == w.ldf && w.L <= 16 && w.S % WG_SP0 == 0 && chunk % WG_SP0 == 0 && w.Np_pad > 0 &&
                       w.Np_pad < (1 << 24) && (chunk + w.Np_pad - 1) / w.Np_pad + 1 <= F0_PATCHES
                   ? WgPick{WG_DMA_F0, 256, 96}
                   : none;
    // LDS-DMA ring: 256-wide dz blocks with a 256-wide (hidden) or 96-wide (layer 0, L = 16) feat
    const bool dma = w.dtype != 0 && w.M % 256 == 0 && w.ldz % 8 == 0 && w.ldz >= w.M && w.S % WG_SPH == 0 &&
                     chunk % WG_SPH == 0 && (long long)w.n_chunks * (w.M / 256) * ((w.K + 255) / 256) <= 0x7fffffff &&
                     dma_enabled;
    const bool dma256 = dma && w.K % 256 == 0 && w.ldf % 8 == 0 && w.ldf >= w.K, dma96 = dma && w.K == 96 && w.ldf == 96;
    if (w.dzl)  // one 256 x 256 block of bf16 T16 tensors
        return dma256 && w.dtype == 1 && w.t16 && !w.ranged && w.M == 256 && w.K == 256 && w.ldz == 256 && w.n_chunks >= 1
                   ? WgPick{WG_DMA_DZL, 256, 256}
                   : none;
    if (w.ranged && !(dma256 || dma96)) return none;  // range mode: the LDS-DMA kernel only
    if (w.t16 && w.dtype == 0) return none;           // T16: 16-bit tensors of the step kernel only
    if (dma256) return {WG_DMA256, 256, 256};
    if (dma96) return {WG_DMA96, 256, 96};
    if (w.M >= 256 && w.K >= 192) return {WG_STAGED, 256, 256};
    if (w.M >= 256 && w.K > 64) return {WG_STAGED, 256, 128};  // layer 0 at L = 16 reads dz once
    return {WG_STAGED, w.M >= 256 ? 256 : 128, 64};
}
// what the kernels did before their conditions were gathered here (each row read off that code)
namespace wg_pinned {
// the C3 hidden layer, row-major: bf16, 256 x 256, S and chunk multiples of 32
constexpr WgShape hidden() {
    WgShape w = {};
    w.dtype = 1;
    w.M = w.ldz = w.K = w.ldf = 256;
    w.S = 4 * 65536;
    w.chunk = 1024;
    w.n_chunks = 256;
    return w;
}
constexpr WgShape prec(WgShape w, int dtype) { return w.dtype = dtype, w; }
constexpr WgShape rows(WgShape w, int M) { return w.M = w.ldz = M, w; }
constexpr WgShape cols(WgShape w, int K) { return w.K = w.ldf = K, w; }
constexpr WgShape stride(WgShape w, int ldf) { return w.ldf = ldf, w; }
constexpr WgShape t16(WgShape w) { return w.t16 = true, w; }
constexpr WgShape planes(WgShape w) { return w.split = true, w; }
constexpr WgShape dzl(WgShape w) { return w.dzl = true, w; }
constexpr WgShape ranged(WgShape w) { return w.ranged = true, w.chunk = 0, w.n_chunks = 28, w; }
constexpr WgShape f0(WgShape w, int L) { return w.f0 = true, w.L = L, w.Np_pad = 65536, cols(w, 96); }
constexpr bool is(const WgShape& w, bool dma, WgKernel k, int bm = 0, int bn = 0) {
    const WgPick p = wg_pick(w, dma);
    return p.k == k && (k != WG_STAGED || (p.bm == bm && p.bn == bn));
}
constexpr WgShape c3 = t16(hidden());  // ... as the step kernel saves it
static_assert(is(c3, true, WG_DMA256), "C3 hidden layer");
static_assert(is(dzl(c3), true, WG_DMA_DZL), "... with dz recomputed");
static_assert(is(prec(c3, 0), true, WG_NONE), "T16 with fp32");
static_assert(is(prec(hidden(), 0), true, WG_STAGED, 256, 256), "C3 hidden layer's shape in fp32");
static_assert(is(c3, false, WG_STAGED, 256, 256), "... with MARF_WGRAD_DMA=0");
static_assert(is(cols(c3, 96), true, WG_DMA96), "K = ldf = 96, bf16");
static_assert(is(cols(c3, 96), false, WG_STAGED, 256, 128), "... with MARF_WGRAD_DMA=0");
static_assert(is(f0(c3, 16), true, WG_DMA_F0) && is(f0(c3, 16), false, WG_DMA_F0), "feat_0 recomputed at L = 16");
static_assert(is(f0(c3, 17), true, WG_NONE), "feat_0 recomputed at L = 17");
static_assert(is(rows(hidden(), 128), true, WG_STAGED, 128, 64), "M = 128");
static_assert(is(cols(rows(hidden(), 512), 512), true, WG_DMA256), "M = 512, K = 512, bf16");
static_assert(is(prec(ranged(c3), 0), true, WG_NONE), "range mode with fp32");
static_assert(is(cols(ranged(c3), 64), true, WG_NONE), "range mode with K = 64");
static_assert(is(ranged(c3), true, WG_DMA256) && is(ranged(c3), false, WG_NONE), "range mode: the LDS-DMA kernel only");
static_assert(is(planes(cols(hidden(), 448)), true, WG_STAGED_SPLIT) && is(planes(cols(hidden(), 448)), false, WG_STAGED_SPLIT),
              "hi + lo planes with K = 448");
static_assert(is(dzl(c3), false, WG_NONE), "dz recomputed: the LDS-DMA kernel only");
static_assert(is(ranged(dzl(c3)), true, WG_NONE), "dz recomputed in range mode");
static_assert(is(prec(c3, 2), true, WG_DMA256) && is(dzl(prec(c3, 2)), true, WG_NONE), "fp16x2");
static_assert(is(cols(hidden(), 64), true, WG_STAGED, 256, 64), "layer 0 at L <= 12, stored");
static_assert(is(stride(hidden(), 260), true, WG_STAGED, 256, 256), "a feat stride the DMA cannot take");
}  // namespace wg_pinned

// MARF_WGRAD_DMA (A/B switch, read here at every call: 0 = register-staged kernels) into wg_pick
WgPick marf_wgrad_pick(const WgShape& w);
hipError_t marf_launch_wgrad(const WgJob& j, hipStream_t s);
// One layer's weight gradient, as every backward lists it: its product (job.dz and glast null: none,
// the partials [n_parts][job.M][job.K] are there already) and the fixed-order reduction of n_parts
// partials into dW [Mo][Ko] / db [Mo]
struct WgLayer {
    WgJob job;
    const float* glast;  // the unfused last layer's product (marf_launch_wgrad_last): glast (x) job.feat over
                         // job.S rows split by job.chunk / n_chunks into job.partial [n_chunks][3][job.K]
    int l;               // the layer (its event, its profile scope)
    int n_parts;         // partials to reduce (with a product: its n_chunks)
    int Mo, Ko;
    float* dW;
    float* db;
    const int* kmap;     // layer 0: column of true input feature k in the partial
    float* scratch;      // where a reduction above 1,024 partials folds them first (null: it never has as many)
};
// The fused launch of a list: every layer on a one-block LDS-DMA 256 kernel (the hidden layers) in
// one launch on s, the one other product (layer 0) beside it on s2 (fork / join events), then every
// layer's reduction in one launch on s; false if a shape does not qualify.  post: the exact power of
// two the products' partials carry the inverse of (2^-10: the fp16x2 recipe)
bool marf_wgrad_fused_ok(const WgLayer* layers, int n_layers);
hipError_t marf_launch_wgrad_fused(const WgLayer* layers, int n_layers, const float* gscale, const float* denom,
                                   hipStream_t s, hipStream_t s2, hipEvent_t fork, hipEvent_t join, float post = 1.f);
hipError_t marf_launch_wgrad_last(int dtype, const float* glast, const void* feat, long long S, int ldf, int K,
                                  int chunk, int n_chunks, float* partial, float* bpartial, hipStream_t s);
hipError_t marf_launch_wgrad_reduce(const float* partial, const float* bpartial, int n_chunks, int M, int K, int Mo,
                                    int Ko, float* dW, float* db, hipStream_t s, const float* gscale = nullptr,
                                    const float* denom = nullptr, float* scratch = nullptr,
                                    const int* kmap = nullptr, float post = 1.f);
hipError_t marf_launch_mask_fwd(const marf::MaskFwdArgs& a, size_t lds, int n_tiles, hipStream_t s);
hipError_t marf_launch_mask_bwd(const marf::MaskBwdArgs& a, size_t lds, int n_tiles, hipStream_t s);
hipError_t marf_launch_mse_mask_bwd(const float* pred, const float* gt, const float* mask, int B, int Np,
                                    const float* stats, const float* gout, float* d_mask, hipStream_t s);
// warp_only (both tile steps): the frozen-image instantiations -- nothing saved for weight gradients,
// no last-layer weight / bias gradient partials (feat / dz / wlast_partial / blast_partial unused)
hipError_t marf_launch_mlp_step(const marf::StepArgs& a, int dtype, int TP, int NW, size_t lds, int n_tiles, hipStream_t s,
                                bool warp_only = false);
// the split tile step of MARF_BF16X3 nets beyond k_step2's reach (marf_step_split.hip); TP 64 or 128
hipError_t marf_launch_mlp_step_split(const marf::StepArgs& a, int TP, bool fwd_only, size_t lds, int n_tiles,
                                      hipStream_t s, bool warp_only = false);
// the Gauss-Newton tile kernel (marf_gn.hip): split = the bf16x3 tile recipe (TP 128 or 64), else fp32
// (TP 64); loss_only: forward, sse and msum only; robust: the IRLS instantiations (a.robust_kind,
// a.robust_delta, a.weight).  Then a patch's tile partials summed in tile order into out [B][56]
// (loss_only: the first two values).
hipError_t marf_launch_gn(const marf::GnArgs& a, bool split, int TP, bool loss_only, size_t lds, int n_tiles,
                          hipStream_t s, bool robust = false);
hipError_t marf_launch_gn_robust(const marf::GnArgs& a, bool split, int TP, bool loss_only, size_t lds, int n_tiles,
                                 hipStream_t s);  // (marf_gn_robust.hip; marf_launch_gn's robust branch)
hipError_t marf_launch_gn_reduce(const double* partial, int tiles_per_patch, int B, bool loss_only, double* out,
                                 hipStream_t s);
hipError_t marf_launch_c2f_weights(const marf::C2fDev& c, int L, float* out, hipStream_t s,
                                   const int* csrc = nullptr, int* cdst = nullptr, int cn = 0);
hipError_t marf_launch_loss_final(const double* part, int n, float* out, const float* denom_override, hipStream_t s);
hipError_t marf_launch_step2(const marf::Step2Args& a, int variant, int grid, hipStream_t s, int full_nk0, bool dz = false);
// the warp-only step (k_step2w: the bf16 split recipe with nothing saved; marf_warp_step_forward)
hipError_t marf_launch_step2_warp(const marf::Step2Args& a, int grid, hipStream_t s, int full_nk0);
hipError_t marf_launch_pack2(const float* params, void* prog, float* bias_out, int* kmap, const marf::Pack2Args& a,
                             hipStream_t s);
hipError_t marf_launch_edge_map(const float* in, double* out, int n_img, int H, int W, hipStream_t s);
hipError_t marf_launch_erode_rect(const float* in, float* out, int n_img, int H, int W, int kh, int kw, hipStream_t s);
hipError_t marf_launch_mse(const float* pred, const float* gt, const float* mask, int B, int Np, double* part,
                           float* out, const float* denom_override, hipStream_t s);
hipError_t marf_launch_mse_bwd(const float* pred, const float* gt, const float* mask, int B, int Np,
                               const float* denom, const float* gout, float* d_pred, hipStream_t s);
hipError_t marf_launch_adam(float* p, const float* g, float* m, float* v, long long n, float w1, float b2,
                            float one_minus_b2, float step_size, float bc2_sqrt, float eps, const float* grad_scale,
                            hipStream_t s);
hipError_t marf_launch_adam_sched(float* p, const float* g, float* m, float* v, long long n, float w1, float b2,
                                  float one_minus_b2, const float* sched, const int* index, float eps,
                                  const float* grad_scale, hipStream_t s);
// dtype 3: the all-operands-split bf16 images (hi [rows][K], then lo, per matrix)
hipError_t marf_launch_pack(int dtype, const float* params, char* packed, const marf::PackArgs& a,
                            long long max_elems, hipStream_t s);
hipError_t marf_launch_pixel_grid(const GeoDev& g, float* xy, int n, hipStream_t s);
hipError_t marf_launch_warp_points(const float* xy, const float* Hm, float* uv, int B, int n, int xy_shared,
                                   hipStream_t s);
hipError_t marf_launch_posenc(const float* coord, long long n, int L, const float* progress, float start, float span,
                              int c2f_on, float* enc, hipStream_t s);
hipError_t marf_launch_warp_points_bwd(const float* xy, const float* Hm, const float* G, float* dxy, float* dH, int B,
                                       int n, int xy_shared, hipStream_t s);
hipError_t marf_launch_posenc_bwd(const float* coord, const float* G, long long n, int L, const float* progress,
                                  float start, float span, int c2f_on, float* dcoord, hipStream_t s);
hipError_t marf_launch_prologue_probe(const GeoDev& g, const marf::C2fDev& c, int L, const float* gt,
                                      const float* mask, float* out, int grid, hipStream_t s);
