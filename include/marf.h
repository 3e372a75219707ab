/*
 * marf.h -- C ABI of libmarf.so, the MI355X (gfx950) implementation of the planar
 * bundle-adjustment render loop of thomasjaron/masking-bundle-adjusting-neural-radiance-fields
 * (model/planar.py + warp.py).
 *
 * The reference has no FFI: its boundary is the Python module API.  Each entry
 * point below replaces the reference interface named in its comment; the Python host package
 * (masking-bundle-adjusting-neural-radiance-fields_amd/marf_hip.py) binds them with ctypes and
 * keeps the reference's module / autograd contract on top.
 *
 * Conventions
 *   - Plain pointers and sizes only.  Every pointer argument named d_* / device is HIP device
 *     memory owned by the caller (PyTorch's allocator); the library borrows it for the call.
 *   - `stream` is a hipStream_t passed as void*; every call is asynchronous on it, no implicit
 *     device synchronisation, no allocation on the step path.
 *   - Every function returns 0 on success or a negative MARF_ERR_* code; marf_last_error()
 *     returns a thread-local message for the last failure.
 *   - float32 everywhere in the interface; dtype selects the internal MLP arithmetic
 *     (MARF_FP32 = exact fp32 MFMA, MARF_BF16 = bf16 MFMA with fp32 accumulation, MARF_BF16X3 = split
 *     bf16, MARF_FP16 = fp16 MFMA with fp32 accumulation, MARF_FP16X2 = split-fp16 weights).
 */
#ifndef MARF_H
#define MARF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MARF_OK 0
#define MARF_ERR_INVALID -1   /* bad argument / shape (reference: AssertionError) */
#define MARF_ERR_HIP -2       /* HIP runtime error */
#define MARF_ERR_UNSUPPORTED -3

#define MARF_FP32 0
#define MARF_BF16 1
#define MARF_BF16X3 2 /* split bf16: weights and forward activations as bf16 hi + lo pairs (hi*hi + hi*lo + lo*hi
                         forward, hi + lo weights in the dgrad), bf16 dz / saved tensors; fused step and
                         marf_render only (marf_forward / marf_backward return MARF_ERR_UNSUPPORTED).
                         Reach: k_step2 up to 5 layers x 256, the split tile kernel beyond, up to 512 wide
                         (no skip layers).  The split tile kernel (k_mlp_step_split, what
                         marf_net_step_kernel names for such a net), with split(x): hi = bf16_rne(x),
                         lo = bf16_rne(x - float(hi)):
                           forward  z = W_h a_h + W_h a_l + W_l a_h, fp32 accumulation
                                    (v_mfma_f32_32x32x16_bf16), the bias as the accumulator's start;
                                    a' = relu(z) split; the layer-0 input is the fp32 prologue's features
                                    split; the last layer's rows in the same three terms; sigmoid, loss
                                    partials and d rgb in fp32
                           dgrad    da = W_h^T dz_h + W_h^T dz_l + W_l^T dz_h, dz = da * relu' split (k_step2
                                    keeps dz single bf16: two terms); the layer-0 adjoint in fp32
                           saved    the hi planes only -- feat_l = a_h, (dz_l)_h, bf16 rows [S][Kp_l] -- and
                                    the ReLU records: plain bf16's bytes per pixel
                           wgrad    the bf16 launchers on the saved hi planes: dW = dz_h^T a_h, fixed-order
                                    split-K
                           packed   every Wf / Wt image as hi then lo (marf_net_packed_bytes: larger) */

#define MARF_FP16 3   /* fp16 MFMA (v_mfma_f32_32x32x16_f16, fp32 accumulation): weights, activations, dz and the
                         saved tensors in IEEE binary16 (11 significant bits); the bf16 rate */
#define MARF_FP16X2 4 /* split-fp16 weights: every MFMA fp16 with the weights as fp16 hi + lo pairs (W_hi a +
                         W_lo a forward, W_hi^T dz + W_lo^T dz dgrad: 2 MFMAs per MAC), activations, dz and
                         the saved tensors single fp16 (dz carrying an exact 2^10 gradient scale); full-width
                         nets (5 layers, every hidden layer 256 wide, 8 <= L <= 16, no skip); fused step and
                         marf_render only */

#define MARF_BF16X3A 5 /* the mask network's all-operands-split bf16 (marf_mask_net_create only; marf_net_create*
                          return MARF_ERR_UNSUPPORTED): every GEMM operand x -- weights, activations, dz -- is
                          hi = bf16_rne(x), lo = bf16_rne(x - hi), every product hi*hi + hi*lo + lo*hi into one fp32
                          accumulator (v_mfma_f32_32x32x16_bf16), in the forward, the dgrad and the weight gradient;
                          saved tensors as hi and lo bf16 planes (the fp32 recipe's bytes per pixel) */

#define MARF_GEO_GRID 0   /* pixels of the centre crop, warped by a per-patch homography */
#define MARF_GEO_COORDS 1 /* explicit [n][2] coordinates (one point set) */
#define MARF_GEO_CANVAS 2 /* every pixel of the H x W canvas (use_cropped_images off), warped per patch
                             (warp.py:54-68 grid; patch_H / patch_W ignored) */

typedef struct marf_net marf_net; /* opaque: MLP shape + padding plan */

typedef struct {
    int mode;             /* MARF_GEO_GRID, MARF_GEO_CANVAS or MARF_GEO_COORDS */
    int B;                /* patches (GRID / CANVAS) ; must be 1 for COORDS */
    int Np;               /* GRID / CANVAS: computed; COORDS: number of points */
    int H, W;             /* canvas (opt.H, opt.W) */
    int patch_H, patch_W; /* crop (opt.patch_H, opt.patch_W) */
    const float* d_H;     /* GRID: [B][3][3] homographies (from marf_sl3_to_SL3) */
    const float* d_coords;/* COORDS: [Np][2] */
} marf_geometry;

typedef struct {
    const float* d_progress; /* fp32 scalar on device (NeuralImageFunction.progress) */
    double start, end;       /* opt.barf_c2f */
    int on;                  /* 0: barf_c2f is None (no band weighting) */
} marf_c2f;

const char* marf_last_error(void);
int marf_version(void);
/* sha1 of the sources the library was built from (build_lib.py embeds it; the host binding refuses
 * a library whose hash differs from the sources next to it). */
const char* marf_source_hash(void);

/* ---- Lie group (warp.py:95-106 Lie.sl3_to_SL3; torch.linalg.matrix_exp semantics).
 * lie_batch: the batch size torch would see (selects torch's path; pass B unless sharded). */
int marf_sl3_to_SL3(const float* d_h, float* d_H, int B, int lie_batch, void* stream);
int marf_sl3_to_SL3_backward(const float* d_h, const float* d_dH, float* d_dh, int B, int lie_batch, void* stream);
/* SE(2) warps (north_star "sl(3)/SE(2)"; an extension: the reference has sl(3) only, warp.py:72-80).
 * se(2) tangent p = (tx, ty, theta) [B][3] -> the sl(3) parameters h [B][8] of the same generator
 * [[0,-theta,tx],[theta,0,ty],[0,0,0]] in warp.py:101-104's layout; marf_sl3_to_SL3(h) is then the
 * SE(2) exponential and every warp / step entry point takes h unchanged.  Backward: dp = adjoint(dh). */
int marf_se2_to_sl3(const float* d_p, float* d_h, int B, void* stream);
int marf_se2_to_sl3_backward(const float* d_dh, float* d_dp, int B, void* stream);

/* ---- Warp (warp.py:33-68 get_normalized_pixel_grid, one copy [n][2]; warp.py:70-81 warp_grid) */
int marf_pixel_grid(int H, int W, int patch_H, int patch_W, int crop, float* d_xy, void* stream);
int marf_warp_points(const float* d_xy, const float* d_H, float* d_uv, int B, int n, int xy_shared, void* stream);

/* ---- Positional encoding + c2f (model/planar.py:451-471): [n][2] -> [n][4L] */
int marf_posenc(const float* d_coord, long long n, int L, const marf_c2f* c2f, float* d_enc, void* stream);

/* Autograd of Warp.warp_grid's point warp (warp.py:70-81): upstream d_G [B][n][2] -> d xy
 * [B][n][2] (per patch even when xy_shared: the caller sums them) and dH [B][3][3] (per-patch sum
 * over points, fp64 accumulation).  dh then follows from marf_sl3_to_SL3_backward. */
int marf_warp_points_backward(const float* d_xy, const float* d_H, const float* d_G, float* d_dxy, float* d_dH, int B,
                              int n, int xy_shared, void* stream);
/* Autograd of NeuralImageFunction.positional_encoding (model/planar.py:451-471): d_G [n][4L] ->
 * d coord [n][2]; the c2f weights are constants (progress carries no gradient). */
int marf_posenc_backward(const float* d_coord, long long n, int L, const marf_c2f* c2f, const float* d_G, float* d_dcoord,
                         void* stream);

/* Measurement only (no reference counterpart): the fused step's per-pixel input side -- target +
 * mask reads (16 B/px), pixel grid, warp, posenc + c2f -- as a standalone launch of `grid` blocks,
 * one float per block into d_out, so the prologue's HBM rate can be timed. */
int marf_prologue_probe(const marf_geometry* geo, const marf_c2f* c2f, int L, const float* d_gt, const float* d_mask,
                        float* d_out, int grid, void* stream);

/* ---- Neural image MLP (model/planar.py:395-449, NeuralImageFunction)
 * dims[0] = 2 + 4L (input), dims[n_layers] = 3, hidden dims arbitrary (padded internally).
 * Flat fp32 parameter vector layout = NeuralImageFunction.mlp parameters in module order:
 * W0 [dims1][dims0], b0 [dims1], W1, b1, ...  (nn.Linear layout). */
int marf_net_create(int n_layers, const int* dims, int L, int dtype, marf_net** out);
/* As marf_net_create, with the pixels one fused step will process on this GPU (0 = unknown; kept for
 * size-dependent kernel choices: the split recipe runs k_step2 at every size today). */
int marf_net_create_hint(int n_layers, const int* dims, int L, int dtype, long long pixels_hint, marf_net** out);
/* As marf_net_create_hint, with skip connections (model/planar.py:419-420, 440-441; opt.arch.skip):
 * bit l of skip_mask makes layer l's input [previous layer's output ; posenc features] (k_in =
 * dims[l] + dims[0] in the flat parameter layout).  Hidden layers 1 .. n_layers-2 only, dims[l] a
 * multiple of 32; the tile kernels (fp32, bf16, fp16) run such nets, the split-bf16 recipe refuses them. */
int marf_net_create_skip(int n_layers, const int* dims, int L, int dtype, long long pixels_hint, unsigned skip_mask,
                         marf_net** out);
void marf_net_destroy(marf_net* net);
long long marf_net_param_count(const marf_net* net);
size_t marf_net_packed_bytes(const marf_net* net);
/* Name of the kernel that runs this net's fused training step ("k_step2" or "k_mlp_step"),
 * fixed at net creation (no reference counterpart: measurement and test bookkeeping). */
const char* marf_net_step_kernel(const marf_net* net);
/* Layer l's parameters in the flat vector: W_l [dims[l+1]][dims[l]] then b_l, from *off, *len floats. */
int marf_net_layer_count(const marf_net* net);
int marf_net_layer_span(const marf_net* net, int l, long long* off, long long* len);
/* Pipelined weight gradients of the fused step (no reference counterpart: scheduling only; the
 * reference's loss.all.backward() at model/planar.py:196 computes the same sums).  mode 0 = off
 * (default; env MARF_PIPE at net creation), 1 = on at any size, -1 = on for large steps.  When on,
 * marf_step_forward runs the step kernel in pieces of piece_tiles tiles on CUs - wg_blocks blocks
 * and the split-K weight-gradient partials of each finished piece on wg_blocks CUs of a second
 * stream; marf_step_backward then only reduces them.  0 = the default size.  Change it between
 * steps only (the saved-buffer layout of a step depends on it).  Measured slower than the
 * sequential step on MI355X: off by default. */
int marf_net_set_pipeline(marf_net* net, int mode, int wg_blocks, int piece_tiles);
/* fp32 master parameters -> MFMA operand layouts (call after every optimizer step). */
int marf_net_pack(const marf_net* net, const float* d_params, void* d_packed, void* stream);

/* Bytes of the activation cache the backward needs, and of the backward scratch. */
size_t marf_saved_bytes(const marf_net* net, const marf_geometry* geo);
size_t marf_workspace_bytes(const marf_net* net, const marf_geometry* geo);

/* Forward (Graph.forward model/planar.py:329-335 for GRID: grid -> warp -> posenc -> MLP;
 * NeuralImageFunction.forward :429 for COORDS).  rgb: [B][Np][3].  d_saved NULL = inference. */
int marf_forward(const marf_net* net, const marf_geometry* geo, const marf_c2f* c2f, const void* d_packed,
                 float* d_rgb, void* d_saved, void* stream);

/* Backward of marf_forward given d loss / d rgb.  Writes (overwrites) d_params (flat, fp32),
 * and d_h [B][8] (GRID, needs d_h_params = the sl(3) warp parameters) or d_coords [Np][2]
 * (COORDS).  Any output pointer may be NULL. */
int marf_backward(const marf_net* net, const marf_geometry* geo, const marf_c2f* c2f, const void* d_packed,
                  const float* d_h_params, int lie_batch, const float* d_rgb_out, const float* d_drgb,
                  const void* d_saved, void* d_workspace, float* d_dparams, float* d_dh, float* d_dcoords,
                  void* stream);

/* Forward-only render (Graph.forward / NeuralImageFunction.forward without autograd,
 * model/planar.py:329-335, 429-449; Model.predict_entire_image :211-217) in the net's recipe: for
 * split-bf16 nets the pixel-per-wave kernel on grid, canvas or explicit-coordinate geometry with a
 * workspace of marf_render_workspace_bytes(); otherwise marf_forward (d_ws unused). */
size_t marf_render_workspace_bytes(const marf_net* net, const marf_geometry* geo);
int marf_render(const marf_net* net, const marf_geometry* geo, const marf_c2f* c2f, const void* d_packed, float* d_rgb,
                void* d_ws, void* stream);

/* ---- Fused training step (grid geometry).  Graph.forward + Graph.mse_loss (model/planar.py:329-336,
 * 382-391) and the backward of both, computed in one pass per pixel tile because the target and
 * mask are known at forward time.  marf_step_forward writes rgb [B][Np][3] (may be NULL), the loss
 * d_loss_out[3] (as marf_masked_mse: loss, denominator, local 3*sum(mask)) and keeps in d_saved
 * (marf_step_saved_bytes) everything the gradient needs, computed for a unit upstream gradient.
 * marf_step_backward turns it into d_params (flat, fp32) and d_dh [B][8] for the upstream gradient
 * *d_gout (device scalar, d loss / d loss_rgb), reading the denominator from d_loss_out[1]. */
size_t marf_step_saved_bytes(const marf_net* net, const marf_geometry* geo);
int marf_step_forward(const marf_net* net, const marf_geometry* geo, const marf_c2f* c2f, const void* d_packed,
                      const float* d_gt, const float* d_mask, const float* d_denom_override, float* d_rgb,
                      float* d_loss_out, void* d_saved, void* stream);
int marf_step_backward(const marf_net* net, const marf_geometry* geo, const void* d_saved, const float* d_h_params,
                       int lie_batch, const float* d_gout, const float* d_loss_out, float* d_dparams, float* d_dh,
                       void* stream);
/* As marf_step_backward; layer_events[l] (hipEvent_t, n_layers entries, NULL entries skipped) is
 * recorded on the stream as soon as layer l's gradient in d_dparams is final.  The layers finish
 * last layer first, layer 0 last (the order a bucketed all-reduce consumes them). */
int marf_step_backward_ev(const marf_net* net, const marf_geometry* geo, const void* d_saved, const float* d_h_params,
                          int lie_batch, const float* d_gout, const float* d_loss_out, float* d_dparams, float* d_dh,
                          void* const* layer_events, void* stream);

/* ---- Warp-only fused step: register patches on a frozen image.  The reference keeps the neural
 * image a module of its own "so it could be checkpointed" (model/planar.py:408); this is the use that
 * anticipates: a trained image is loaded, its parameters do not move, and further patches (new views,
 * a second batch, a re-registration after a bad start) are aligned to it.  marf_warp_step_forward is
 * marf_step_forward with the same contract for d_rgb (may be NULL) and d_loss_out[3] and the same
 * bits in both, on kernels that keep nothing for weight gradients: d_saved
 * (marf_warp_step_saved_bytes) holds the dH partials (36 B per 32 pixel slots), the per-block loss
 * partials and the band weights -- on the tile kernels also the ReLU records their own dgrad
 * re-reads -- and no feat_l, dz_l, last-layer weight / bias partials or split-K partials.
 * marf_warp_step_backward is the fixed-order sum of the dH partials and the Lie backward into d_dh
 * [B][8] (the bits marf_step_backward gives), on the caller's stream alone: no side stream, no events.
 * The pipelined mode (marf_net_set_pipeline) is ignored: there is no weight-gradient work to overlap.
 * MARF_STEP2_GRID is honoured as by marf_step_forward.  MARF_FP16X2 nets and nets created under
 * MARF_STEP2_DZ=1 or MARF_STEP2=1 have no warp-only kernel: MARF_ERR_UNSUPPORTED with the reason
 * (marf_warp_step_saved_bytes returns 0 and sets it). */
size_t marf_warp_step_saved_bytes(const marf_net* net, const marf_geometry* geo);
int marf_warp_step_forward(const marf_net* net, const marf_geometry* geo, const marf_c2f* c2f, const void* d_packed,
                           const float* d_gt, const float* d_mask, const float* d_denom_override, float* d_rgb,
                           float* d_loss_out, void* d_saved, void* stream);
int marf_warp_step_backward(const marf_net* net, const marf_geometry* geo, const void* d_saved, const float* d_h_params,
                            int lie_batch, const float* d_gout, const float* d_loss_out, float* d_dh, void* stream);

/* ---- Gauss-Newton normal equations of the registration problem on a frozen image (an extension: the
 * reference walks the warps downhill with Adam, model/planar.py:98-99).  With the image frozen the B
 * patches are independent 8-parameter non-linear least-squares problems.  Per patch b and real pixel q,
 * with p the sigmoid output, g the target, m the mask:
 *     r_qc = m_q (p_qc - g_qc)        J_qc = m_q d p_qc / d vec(H_b)   (a row of 9, H_b row-major)
 * marf_gn_normal writes d_out[b] = [sse = sum r^2, msum = sum m, g9 = sum_qc J_qc^T r_qc (9), N = sum_qc
 * J_qc^T J_qc (9 x 9 symmetric: the upper triangle, row-major, 45 values)] in fp64, and rgb [B][Np][3]
 * (may be NULL); with loss_only the forward alone runs and only sse and msum are written, with the full
 * launch's bits.  One tile kernel carries the three channel gradients down the dgrad chain and sums a
 * 56-value partial per tile, a second sums a patch's partials, both in a fixed order without atomics:
 * two calls on the same inputs give the same bits.  The chain to the tangent (d vec(H) / d h from
 * marf_sl3_to_SL3_backward) and the solver are the caller's (marf_hip.gn_normal, model/planar.py).
 * The image's weights are packed once into a buffer of the feature's own (marf_gn_packed_bytes /
 * marf_gn_pack): the fp32 tile layouts, or for a MARF_BF16X3 net -- one in k_step2's reach included --
 * the tile layouts with every image as hi then lo; the arithmetic is exact fp32 MFMA, or the split tile
 * recipe's three terms in the forward and the dgrad.  d_scratch (marf_gn_scratch_bytes) holds the
 * ReLU records, the tile partials and the band weights.  MARF_ERR_UNSUPPORTED with the reason (the
 * byte counts: 0 and the reason in marf_last_error) for MARF_BF16, MARF_FP16 and MARF_FP16X2 nets (a
 * 16-bit Jacobian misses the warp gradient's bound), skip nets, MARF_GEO_COORDS, and a shape whose
 * tile does not fit LDS (marf_gn_scratch_bytes / marf_gn_normal). */
size_t marf_gn_packed_bytes(const marf_net* net);
int marf_gn_pack(const marf_net* net, const float* d_params, void* d_gn_packed, void* stream);
size_t marf_gn_scratch_bytes(const marf_net* net, const marf_geometry* geo);
int marf_gn_normal(const marf_net* net, const marf_geometry* geo, const marf_c2f* c2f, const void* d_gn_packed,
                   const float* d_gt, const float* d_mask, int loss_only, float* d_rgb, double* d_out, void* d_scratch,
                   void* stream);

/* ---- Robust Gauss-Newton: iteratively reweighted least squares (IRLS) on the same problem, for a view
 * with an occluder and no mask of it.  With r, J, m as above, e_q = sum_c r_qc^2, s_q = sqrt(e_q) and a
 * scale delta > 0 in pixel-value units:
 *     MARF_GN_HUBER :  rho(e) = e if e <= delta^2, else 2 delta s - delta^2;   w = 1, else delta / s
 *     MARF_GN_CAUCHY:  rho(e) = delta^2 log1p(e / delta^2);                     w = 1 / (1 + e / delta^2)
 * marf_gn_normal_robust writes d_out[b] = [cost = sum_q rho(e_q), msum = sum_q m_q (unweighted), g9 =
 * sum_q w_q sum_c J_qc^T r_qc, N = sum_q w_q sum_c J_qc^T J_qc (upper triangle)]: the same 56 doubles, the
 * same reduce, Triggs' first-order Hessian (no second-order term of rho), and d cost_b / d vec(H_b) = 2
 * g9_b exactly.  d_weight [B][Np] fp32 (may be NULL) receives w_q of every real pixel, in the loss-only
 * launch too: at the solution it is the view's inlier map.  d_rgb may be NULL.  The weight enters as
 * sqrt(w) on the stored r and m of a slot, so w = 1 changes no bit: MARF_GN_HUBER with delta^2 at or above
 * every e_q gives marf_gn_normal's 56 values and rgb bit for bit.  The packed buffer (marf_gn_pack) and the
 * scratch (marf_gn_scratch_bytes) are marf_gn_normal's, as are its refusals and their reasons; in
 * addition MARF_ERR_INVALID with the reason for an unknown kind and for a delta that is not finite or not
 * > 0.  Two calls on the same inputs give the same bits; loss_only gives the full launch's cost bits. */
#define MARF_GN_HUBER 1
#define MARF_GN_CAUCHY 2
int marf_gn_normal_robust(const marf_net* net, const marf_geometry* geo, const marf_c2f* c2f, const void* d_gn_packed,
                          const float* d_gt, const float* d_mask, int loss_only, int kind, float delta, float* d_rgb,
                          float* d_weight, double* d_out, void* d_scratch, void* stream);

/* ---- MLP-gradient exchange of the patch-sharded step (the reference is
 * single-GPU, options.py:117-120, so this replaces no reference call: it is the one collective the
 * sharding adds).  RCCL over xGMI, librccl.so opened at first use.  marf_comm_unique_id fills 128
 * bytes on one rank (the host shares them with the others); marf_comm_create joins rank `rank` of
 * `nranks` on `device`.  marf_allreduce_grads sums a flat fp32 gradient in place on `stream`;
 * marf_allreduce_grads_layers sums each layer's span (marf_net_layer_span) on the communicator's
 * own stream after its marf_step_backward_ev event, so the exchange overlaps the remaining weight
 * gradients, and makes `stream` wait for the last one.  A NULL entry of layer_events waits for the
 * work queued on `stream` before the call.  marf_comm_create leaves the calling thread's current
 * device unchanged.  After an error from either all-reduce call the ranks' collective sequences may
 * disagree: destroy the communicator (every rank) rather than reuse it. */
typedef struct marf_comm marf_comm;
int marf_comm_unique_id(void* out, size_t cap);
int marf_comm_create(const void* unique_id, int nranks, int rank, int device, marf_comm** out);
void marf_comm_destroy(marf_comm* comm);
int marf_allreduce_grads(marf_comm* comm, float* d_flat, size_t n, void* stream);
int marf_allreduce_grads_layers(marf_comm* comm, const marf_net* net, float* d_dparams, void* const* layer_events,
                                void* stream);

/* ---- Masked MSE (Graph.mse_loss, model/planar.py:382-391).  pred [B][Np][3] (MLP layout),
 * gt [B][3][Np], mask [B][1][Np] or NULL (plain mean).  d_out[3]: loss, denominator used,
 * local 3*sum(mask).  d_denom_override: optional device scalar (global denominator of a patch
 * shard).  d_ws: marf_mse_workspace_bytes(). */
size_t marf_mse_workspace_bytes(void);
int marf_masked_mse(const float* d_pred, const float* d_gt, const float* d_mask, int B, int Np,
                    const float* d_denom_override, float* d_out, void* d_ws, void* stream);
int marf_masked_mse_backward(const float* d_pred, const float* d_gt, const float* d_mask, int B, int Np,
                             const float* d_denom, const float* d_gout, float* d_dpred, void* stream);

/* Gradient of the masked MSE with respect to a soft (learned, non-binary) mask: Graph.mse_loss's
 * autograd into `masks` (model/planar.py:388-390, reached from :362-365 when use_implicit_mask).
 * loss = sum((p - g) m)^2 / (3 sum m), so d loss / d m_q = (2 m_q e_q - 3 loss) / denominator with
 * e_q = sum_c (p - g)^2.  d_stats: the [loss, denominator, .] triple marf_step_forward / marf_masked_mse
 * wrote; d_gout: device scalar upstream gradient; d_dmask [B][1][Np].  No host round trip. */
int marf_masked_mse_mask_backward(const float* d_pred, const float* d_gt, const float* d_mask, int B, int Np,
                                  const float* d_stats, const float* d_gout, float* d_dmask, void* stream);

/* ---- Implicit mask network (model/planar.py:319-327 construction, :340-352 input and forward,
 * :475-488 ImplicitMask, :491-518 PosEmbedding).  Per pixel q of patch b the input is
 * [E[r_q] ; E[g_q] ; E[b_q] ; uv_q]: three rows of the embedding table E [n_vocab][embed_dim]
 * (embedding_view.weight) chosen by d_index [B][3][Np] (int32; images.rgb[b].long()), and uv =
 * [x, y, sin(2^k x), sin(2^k y), cos(2^k x), cos(2^k y)]_{k < n_freqs} of the unwarped grid point of the
 * geometry (grid or canvas; d_H unused).  The MLP is Linear+ReLU x (n_layers - 1), Linear(width, 1),
 * sigmoid; flat fp32 parameters in module order W0 [width][3 embed_dim + 2 + 4 n_freqs], b0, W1, b1, ...
 * (mask_mapping.{0,2,..}.{weight,bias}).  dtype: MARF_FP32 (exact fp32 MFMA) or MARF_BF16X3A (every operand
 * split into bf16 hi + lo; ~1e-5 of max on the gradients); MARF_BF16 / BF16X3 / FP16 / FP16X2 return
 * MARF_ERR_UNSUPPORTED: plain bf16 missed the 1e-2 bound on the weight gradients and the image net's single-bf16
 * dz sits on it.  MARF_BF16X3A packs each matrix as a hi and a lo bf16 image (packed_bytes: two
 * bf16 planes per matrix); its saved / workspace buffers hold hi and lo [S][Kp] bf16 planes per tensor and are
 * as large as the fp32 recipe's.
 * The reference's defaults are embed_dim 128, n_freqs 10, width 256, n_layers 5 (306,945 parameters). */
typedef struct marf_mask_net marf_mask_net;
int marf_mask_net_create(int n_vocab, int embed_dim, int n_freqs, int width, int n_layers, int dtype,
                         marf_mask_net** out);
void marf_mask_net_destroy(marf_mask_net* net);
long long marf_mask_net_param_count(const marf_mask_net* net);
size_t marf_mask_net_packed_bytes(const marf_mask_net* net);
/* fp32 master parameters -> MFMA operand layouts (after every optimizer step). */
int marf_mask_net_pack(const marf_mask_net* net, const float* d_params, void* d_packed, void* stream);
size_t marf_mask_saved_bytes(const marf_mask_net* net, const marf_geometry* geo);
size_t marf_mask_workspace_bytes(const marf_mask_net* net, const marf_geometry* geo);
/* m [B][1][Np] (the layout marf_step_forward reads its mask in; var.mask_prediction [B, Np, 1] is the
 * same memory).  d_saved NULL = inference; else marf_mask_saved_bytes() for the backward. */
int marf_mask_forward(const marf_mask_net* net, const marf_geometry* geo, const void* d_packed, const float* d_embed,
                      const int* d_index, float* d_m, void* d_saved, void* stream);
/* Backward given d loss / d m [B][1][Np]: overwrites d_dparams (flat, fp32).  No gradient for the
 * embedding table: the reference puts embedding_view in no optimizer group (model/planar.py:93-96),
 * so layer 0's input gradient is never needed.  d_workspace: marf_mask_workspace_bytes(). */
int marf_mask_backward(const marf_mask_net* net, const marf_geometry* geo, const void* d_packed, const float* d_m,
                       const float* d_dm, const void* d_saved, void* d_workspace, float* d_dparams, void* stream);

/* ---- Edge maps (inputs.compute_edges, reference inputs.py:50-67: cv2.Sobel 3x3 CV_64F in x and y,
 * magnitude, cv2.GaussianBlur 5x5 sigma 0, BORDER_REFLECT_101), per channel image on the device.
 * d_img [n_img][H][W] fp32 -> d_out [n_img][H][W] fp64. */
int marf_edge_map(const float* d_img, int n_img, int H, int W, double* d_out, void* stream);

/* ---- Mask erosion (erode_images, reference inputs.py:71-85: cv2.erode with a kh x kw MORPH_RECT
 * element, default anchor and border).  d_img [n_img][H][W] fp32 -> d_out (a different buffer). */
int marf_erode_rect(const float* d_img, int n_img, int H, int W, int kh, int kw, float* d_out, void* stream);

/* ---- Mosaic of the registered patches (an extension: the reference's only image is the neural image's own
 * render, model/planar.py:211-217).  Every input patch is inverse-warped onto the canvas and blended; per
 * canvas pixel the call reports the blended colour, the total weight, the number of contributing patches and
 * the disagreement between them.
 *
 * Geometry is marf_pixel_grid's: canvas H x W; patch h x w = the crop window of (patch_H, patch_W) if crop
 * (rows [y0, y0 + h) with y0 = H/2 - patch_H/2, h = (H/2 + patch_H/2) - y0 in integers, columns likewise: for even
 * sizes h = patch_H, w = patch_W), else the canvas with y0 = x0 = 0; norm_w = W / max(H, W), norm_h = H / max(H, W);
 * grid(k, n, norm) = ((k + 0.5) / n * 2 - 1) * norm.  For canvas pixel (i, j) and each patch b in index order:
 *     y = (grid(j, W, norm_w), grid(i, H, norm_h));   (X0, X1, X2) = Hinv_b (y, 1);
 *     (x, y~) = (X0, X1) / (X2 + 1e-8)                                      (marf_warp_points' arithmetic)
 *     c = (x / norm_w + 1) W / 2 - 0.5 - x0,   r = (y~ / norm_h + 1) H / 2 - 0.5 - y0
 * Patch b contributes iff X2 > 0 and -E <= c <= w - 1 + E and -E <= r <= h - 1 + E with E = 2^-10 px; c and r are
 * then clamped to [0, w-1] and [0, h-1].  (E belongs to the definition: an identity warp puts the patch's border
 * pixels on c = 0 exactly, and without E fp32 rounding would decide whether they are inside.)
 *     v_b  = bilinear sample of d_img[b] (three channels) at (r, c)
 *     m_b  = bilinear sample of d_weight[b] at (r, c); 1 if d_weight is NULL
 *     f_b  = max(2^-10, (1 - |2c/(w-1) - 1|)(1 - |2r/(h-1) - 1|)) if feather, else 1
 *     om_b = f_b m_b
 * Outputs:  count = number of contributing patches with om_b > 0;  wsum = sum om_b;
 *     image = sum om_b v_b / wsum (0 in all three channels where wsum == 0);
 *     var   = sum om_b |v_b - image|^2 / (3 wsum): the mean over channels, >= 0, and 0 where count < 2.
 * image and var accumulate in fp32 in patch order by a weighted Welford update (never as sum om v^2 / wsum -
 * mean^2, which cancels); no atomics: two calls on the same inputs give the same bits.  d_weight = NULL gives
 * the bits of an explicit map of ones; d_count / d_var = NULL change no bit of d_image and d_wsum.
 * Hinv_b is the caller's: marf_sl3_to_SL3(-h_b), the exact inverse of expm(A(h_b)) (se2: of the embedded
 * parameters).  Weights are expected >= 0: a contribution whose om_b is not > 0 (zero, negative, NaN) is left
 * out of every output, wsum included.  MARF_ERR_INVALID with the reason, before any HIP call: a NULL d_Hinv /
 * d_img / d_image / d_wsum, B < 1, non-positive sizes, a canvas side above 16384 (beyond it fp32 no longer holds
 * the tolerance E beside w - 1), a patch larger than the canvas, feather with h < 2 or w < 2. */
int marf_compose(int H, int W, int patch_H, int patch_W, int crop, int B,
                 const float* d_Hinv   /* [B][9] row-major */,
                 const float* d_img    /* [B][3][h*w]      */,
                 const float* d_weight /* [B][1][h*w] or NULL = ones */,
                 int feather,
                 float* d_image /* [3][H*W] */, float* d_wsum /* [H*W] */,
                 float* d_count /* [H*W] or NULL */, float* d_var /* [H*W] or NULL */,
                 void* stream);

/* ---- Adam (torch.optim.Adam, model/planar.py:98-99): one parameter segment, step >= 1.
 * d_grad_scale: optional device scalar multiplying the gradient (NULL = 1). */
int marf_adam_step(float* d_p, const float* d_g, float* d_m, float* d_v, long long n, double lr, double beta1,
                   double beta2, double eps, long long step, const float* d_grad_scale, void* stream);
/* The same update with the step's scalars read on the device, so a captured training iteration
 * (Model.captured_step) replays it without host values: marf_adam_schedule fills h_out[2 i],
 * h_out[2 i + 1] with step_size = lr / (1 - beta1^k) and sqrt(1 - beta2^k) for k = first_step + i,
 * exactly as marf_adam_step computes them (host only); marf_adam_step_sched reads row *d_index of
 * that table (uploaded by the caller) on the stream. */
int marf_adam_schedule(double lr, double beta1, double beta2, long long first_step, long long count, float* h_out);
int marf_adam_step_sched(float* d_p, const float* d_g, float* d_m, float* d_v, long long n, double beta1, double beta2,
                         double eps, const float* d_sched, const int* d_index, const float* d_grad_scale, void* stream);

/* ---- Profiling: HIP events recorded around each kernel on its launch stream (off by default).
 * marf_profile_read drains the recorded pairs (synchronising on them) and returns, per kernel
 * name, the summed duration (ms) and launch count; names is a [cap][name_len] char array. */
int marf_profile_enable(int on);
/* Restrict the timing to the kernels named in `names` (comma-separated profile names, e.g.
 * "mlp_step"; NULL or "" = every kernel), so a timed region pays for the event pairs of the kernels
 * it reports only (each pair adds a few microseconds between launches). */
int marf_profile_filter(const char* names);
int marf_profile_reset(void);
int marf_profile_read(char* names, int name_len, double* total_ms, long long* count, int cap);

/* ---- Diagnostics: device buffer [n_tiles][32] (u64) receiving the fused step's per-phase
 * s_memtime stamps; only a library built with -DMARF_STAMPS writes it (tools/phase_stamps.py). */
void marf_debug_set_stamps(void* d_stamps);

#ifdef __cplusplus
}
#endif
#endif /* MARF_H */
