// marf_compose.hip -- the mosaic of the registered patches (include/marf.h marf_compose).
//
// Every input patch is inverse-warped onto the H x W canvas with the caller's inverse homographies
// (sl3_to_SL3(-h_b)) and blended per canvas pixel: colour, total weight, number of contributing patches
// and the weighted disagreement between them.  The reference has no such stage (its only image is the
// neural image's own render, model/planar.py:211-217); the geometry is marf_pixel_grid's.
//
// One thread per canvas pixel, 16 x 16 blocks (k_edge_map's tiling: a block's taps into a patch are a
// compact window the L1 / L2 serve).  The [B][9] matrices are block-uniform: they go to LDS once per
// block, MARF_COMPOSE_CHUNK patches at a time, and beside them one flag per patch -- the block-level
// early-out: a patch whose window provably misses the block's canvas tile is skipped by the whole
// block.  The flag only ever drops patches no pixel of the tile accepts, so the result bits do not depend
// on it (-DMARF_COMPOSE_EARLY_OUT=0 builds the kernel without it for the A/B).  Patches are visited in
// index order; mean and disagreement accumulate in fp32 by West's weighted update (no sum of squares
// minus squared mean), so two launches give the same bits.  No atomics; per-lane vector loads and stores.
// Bound: memory / latency: 16 B out per canvas pixel, 16 taps of 4 B per contributing patch.
#include "marf_args.h"

#ifndef MARF_COMPOSE_EARLY_OUT
#define MARF_COMPOSE_EARLY_OUT 1
#endif
#define MARF_COMPOSE_CHUNK 64

namespace marf {

struct ComposeArgs {
    int H, W;        // canvas
    int h, w;        // patch (the crop window, or the canvas)
    int x0, y0;      // crop origin on the canvas (0 without crop)
    int B;
    int feather;
    float norm_h, norm_w;
    const float* Hinv;    // [B][9]
    const float* img;     // [B][3][h*w]
    const float* weight;  // [B][1][h*w] or null (ones)
    float* image;         // [3][H*W]
    float* wsum;          // [H*W]
    float* count;         // [H*W] or null
    float* var;           // [H*W] or null
};

constexpr float kComposeE = 0.0009765625f;  // 2^-10 px: the validity tolerance and the feather floor

// Canvas pixel coordinates of a warped point: c = (u / norm_w + 1) W / 2 - 0.5 - x0, r likewise.
MARF_DEV float patch_coord(float u, float norm, int dim, int o) {
    float t = u / norm;
    t = t + 1.0f;
    t = t * (float)dim;
    t = t * 0.5f;
    t = t - 0.5f;
    return t - (float)o;
}

// a + f (b - a): a constant row gives the constant back exactly (a NULL weight and a map of ones agree bit for bit)
MARF_DEV float lerp(float a, float b, float f) { return a + f * (b - a); }

// May the whole block skip this patch?  Only if every pixel of its canvas tile provably fails the
// validity test.  The tile's pixel centres lie in the convex hull of its four corner centres; where
// the homogeneous coordinate X2 is positive at the four corners (and not the result of a cancellation:
// X2 >= 2^-10 of the sum of its terms' magnitudes, so its relative rounding error is below 2^-13) it is
// positive on the hull and the projective image of the hull is the hull of the images, so every
// pixel's (c, r) lies in the corners' bounding box up to rounding.  The margin -- one pixel plus 2^-8
// of the largest coordinate magnitude in play -- is orders above that rounding.  NaN / Inf fail every
// comparison and keep the patch.
MARF_DEV bool tile_misses_patch(const ComposeArgs& a, const float* Hm, int jA, int iA) {
    const int jB = min(jA + 15, a.W - 1), iB = min(iA + 15, a.H - 1);
    float cmin = INFINITY, cmax = -INFINITY, rmin = INFINITY, rmax = -INFINITY;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float x = grid_coord((k & 1) ? jB : jA, a.W, a.norm_w);
        const float y = grid_coord((k & 2) ? iB : iA, a.H, a.norm_h);
        float X[3], u, v;
        warp_point(Hm, x, y, u, v, X);
        const float mag = (fabsf(x * Hm[6]) + fabsf(y * Hm[7])) + fabsf(Hm[8]);
        ok = ok && (X[2] >= mag * kComposeE) && (X[2] > 0.0f);
        const float c = patch_coord(u, a.norm_w, a.W, a.x0), r = patch_coord(v, a.norm_h, a.H, a.y0);
        cmin = fminf(cmin, c);
        cmax = fmaxf(cmax, c);
        rmin = fminf(rmin, r);
        rmax = fmaxf(rmax, r);
        ok = ok && (fabsf(c) < INFINITY) && (fabsf(r) < INFINITY);
    }
    float big = fmaxf(fmaxf(fabsf(cmin), fabsf(cmax)), fmaxf(fabsf(rmin), fabsf(rmax)));
    big = fmaxf(big, (float)max(a.W, a.H));
    const float M = 1.0f + big * 0.00390625f;
    return ok && (cmax < -M || cmin > (float)(a.w - 1) + M || rmax < -M || rmin > (float)(a.h - 1) + M);
}

__global__ __launch_bounds__(256) void k_compose(const ComposeArgs a) {
    __shared__ float sH[MARF_COMPOSE_CHUNK * 9];
    __shared__ int sSkip[MARF_COMPOSE_CHUNK];
    const int tid = threadIdx.x;
    const int j = blockIdx.x * 16 + (tid & 15), i = blockIdx.y * 16 + (tid >> 4);
    const bool active = j < a.W && i < a.H;
    const float gx = grid_coord(j, a.W, a.norm_w), gy = grid_coord(i, a.H, a.norm_h);
    const size_t np = (size_t)a.h * a.w;
    const float wm1 = (float)(a.w - 1), hm1 = (float)(a.h - 1);

    float mean0 = 0.0f, mean1 = 0.0f, mean2 = 0.0f;  // weighted mean of the contributions so far
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;           // sum of omega |v - mean|^2 per channel
    float wsum = 0.0f;
    int cnt = 0;

    for (int b0 = 0; b0 < a.B; b0 += MARF_COMPOSE_CHUNK) {
        const int nb = min(MARF_COMPOSE_CHUNK, a.B - b0);
        if (b0) __syncthreads();  // the previous chunk's readers are done
        for (int e = tid; e < nb * 9; e += 256) sH[e] = a.Hinv[(size_t)b0 * 9 + e];
        if (tid < nb) {
#if MARF_COMPOSE_EARLY_OUT
            sSkip[tid] = tile_misses_patch(a, a.Hinv + (size_t)(b0 + tid) * 9, blockIdx.x * 16, blockIdx.y * 16) ? 1 : 0;
#else
            sSkip[tid] = 0;
#endif
        }
        __syncthreads();
        if (!active) continue;
        for (int bb = 0; bb < nb; ++bb) {
            if (sSkip[bb]) continue;  // block-uniform
            float X[3], u, v;
            warp_point(sH + 9 * bb, gx, gy, u, v, X);
            float c = patch_coord(u, a.norm_w, a.W, a.x0), r = patch_coord(v, a.norm_h, a.H, a.y0);
            // (positive comparisons: a NaN coordinate contributes nothing)
            const bool valid = X[2] > 0.0f && c >= -kComposeE && c <= wm1 + kComposeE && r >= -kComposeE && r <= hm1 + kComposeE;
            if (!valid) continue;
            c = fminf(fmaxf(c, 0.0f), wm1);
            r = fminf(fmaxf(r, 0.0f), hm1);
            const int c0 = (int)c, r0 = (int)r;  // in [0, w-1] x [0, h-1] after the clamp
            const int c1 = min(c0 + 1, a.w - 1), r1 = min(r0 + 1, a.h - 1);
            const float fx = c - (float)c0, fy = r - (float)r0;
            const size_t o00 = (size_t)r0 * a.w + c0, o01 = (size_t)r0 * a.w + c1;
            const size_t o10 = (size_t)r1 * a.w + c0, o11 = (size_t)r1 * a.w + c1;
            const size_t pb = (size_t)(b0 + bb);
            float m = 1.0f;
            if (a.weight) {
                const float* wp = a.weight + pb * np;
                m = lerp(lerp(wp[o00], wp[o01], fx), lerp(wp[o10], wp[o11], fx), fy);
            }
            float f = 1.0f;
            if (a.feather) {
                float fc = (2.0f * c) / wm1;
                fc = 1.0f - fabsf(fc - 1.0f);
                float fr = (2.0f * r) / hm1;
                fr = 1.0f - fabsf(fr - 1.0f);
                f = fmaxf(kComposeE, fc * fr);
            }
            const float om = f * m;
            if (!(om > 0.0f)) continue;
            const float* ip = a.img + pb * 3 * np;
            const float v0 = lerp(lerp(ip[o00], ip[o01], fx), lerp(ip[o10], ip[o11], fx), fy);
            ip += np;
            const float v1 = lerp(lerp(ip[o00], ip[o01], fx), lerp(ip[o10], ip[o11], fx), fy);
            ip += np;
            const float v2 = lerp(lerp(ip[o00], ip[o01], fx), lerp(ip[o10], ip[o11], fx), fy);
            // West's update: mean += (om / wnew) d, S += wsum_old d ((om / wnew) d): every term >= 0
            const float wnew = wsum + om;
            const float q = om / wnew;
            const float d0 = v0 - mean0, d1 = v1 - mean1, d2 = v2 - mean2;
            const float t0 = q * d0, t1 = q * d1, t2 = q * d2;
            mean0 = mean0 + t0;
            mean1 = mean1 + t1;
            mean2 = mean2 + t2;
            s0 = s0 + wsum * (d0 * t0);
            s1 = s1 + wsum * (d1 * t1);
            s2 = s2 + wsum * (d2 * t2);
            wsum = wnew;
            ++cnt;
        }
    }
    if (!active) return;
    const size_t HW = (size_t)a.H * a.W, p = (size_t)i * a.W + j;
    a.image[p] = mean0;  // (0 where nothing contributed)
    a.image[HW + p] = mean1;
    a.image[2 * HW + p] = mean2;
    a.wsum[p] = wsum;
    if (a.count) a.count[p] = (float)cnt;
    if (a.var) a.var[p] = cnt >= 2 ? ((s0 + s1) + s2) / (3.0f * wsum) : 0.0f;
}

}  // namespace marf

using namespace marf;

hipError_t marf_launch_compose(int H, int W, int h, int w, int x0, int y0, float norm_h, float norm_w, int B,
                               const float* Hinv, const float* img, const float* weight, int feather, float* image,
                               float* wsum, float* count, float* var, hipStream_t s) {
    ComposeArgs a;
    a.H = H;
    a.W = W;
    a.h = h;
    a.w = w;
    a.x0 = x0;
    a.y0 = y0;
    a.B = B;
    a.feather = feather;
    a.norm_h = norm_h;
    a.norm_w = norm_w;
    a.Hinv = Hinv;
    a.img = img;
    a.weight = weight;
    a.image = image;
    a.wsum = wsum;
    a.count = count;
    a.var = var;
    dim3 grid((W + 15) / 16, (H + 15) / 16, 1);
    hipLaunchKernelGGL(k_compose, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}
