// What the workgroup-per-tile 3DGS rasterizers (rasterize.hip: tile sizes other
// than 16; rasterize_wide.hip: 33..512 channels) agree on: the compositing
// constants, the argument block, the walk from a workgroup to its tile, pixels
// and isect range, the staging of a batch's geometry, and the per-record
// alpha step of the forward and of the backward.  A header, so that each file
// compiles it under its own flags (csrc/Makefile).  Every other rasterizer
// (raster16.h, rasterize_score.hip, indices.hip, surfel) takes the constants.
//
// The rule: alpha = min(kAlphaMax, opacity * exp(-sigma)); a record is blended
// iff sigma >= 0 and alpha >= kAlphaMin; a pixel stops, without blending the
// record, when its transmittance would drop to T <= kTMin.
#pragma once

#include "common.h"

namespace gs {

constexpr float kAlphaMin = 1.f / 255.f;
constexpr float kAlphaMax = 0.999f;
constexpr float kTMin = 1e-4f;

struct TileArgs {
  int C, D, W, H, tw, th, n_tiles, ts;  // ts last: the wide kernels' former layout, DESIGN 3.28
  int64_t n_isects;
  const float *means2d, *conics, *colors, *opacities, *backgrounds;  // backgrounds nullable
  const uint8_t *masks;                                              // nullable
  const int32_t *offsets, *flatten_ids;
  // forward outputs / backward inputs
  float *render_colors, *render_alphas;
  int32_t *last_ids;
  // backward
  const float *v_render_colors, *v_render_alphas;                // alphas nullable
  float *v_means2d, *v_conics, *v_colors, *v_opacities, *v_abs;  // abs nullable
};

// The block from the C ABI's parameters; the backward casts its const inputs at the call.
inline TileArgs tile_args(int C, int D, int W, int H, int ts, int tw, int th, const float *means2d,
                          const float *conics, const float *colors, const float *opacities,
                          const float *backgrounds, const uint8_t *masks, const int32_t *offsets,
                          int64_t n_isects, const int32_t *flatten_ids, float *render_colors,
                          float *render_alphas, int32_t *last_ids,
                          const float *v_render_colors = nullptr,
                          const float *v_render_alphas = nullptr, float *v_means2d = nullptr,
                          float *v_conics = nullptr, float *v_colors = nullptr,
                          float *v_opacities = nullptr, float *v_abs = nullptr) {
  return TileArgs{C, D, W, H, tw, th, C * tw * th, ts, n_isects, means2d, conics, colors,
                  opacities, backgrounds, masks, offsets, flatten_ids, render_colors,
                  render_alphas, last_ids, v_render_colors, v_render_alphas, v_means2d, v_conics,
                  v_colors, v_opacities, v_abs};
}

// The gradient buffers are zeroed (on `st`) before the backward accumulates.
inline int zero_grads(const TileArgs &a, int64_t n_gaussians, hipStream_t st) {
  const size_t G = (size_t)n_gaussians;
  GS_HIP(zero_async(a.v_means2d, sizeof(float) * 2 * G, st));
  GS_HIP(zero_async(a.v_conics, sizeof(float) * 3 * G, st));
  GS_HIP(zero_async(a.v_colors, sizeof(float) * a.D * G, st));
  GS_HIP(zero_async(a.v_opacities, sizeof(float) * G, st));
  if (a.v_abs) GS_HIP(zero_async(a.v_abs, sizeof(float) * 2 * G, st));
  return 0;
}

// The size tests of every entry point; `who` heads the message.
inline int check_tile_sizes(const char *who, int C, int W, int H, int ts, int tw, int th) {
  GS_REQUIRE(C >= 0 && W >= 0 && H >= 0, "%s: negative sizes", who);
  GS_REQUIRE((int64_t)tw * ts >= W && (int64_t)th * ts >= H,
             "%s: tile grid %dx%d x %d does not cover %dx%d", who, tw, th, ts, W, H);
  return 0;
}

// Isect count and the end of tile t's isect range.  Capacity mode (n_dev
// non-null, the sync-free isect of a captured training step): the arrays
// hold n slots, the count is read on the device.
GS_INLINE int64_t isect_count(const int64_t *n_dev, int64_t n) { return n_dev ? *n_dev : n; }
GS_INLINE int64_t tile_end(const int32_t *offsets, int t, int n_tiles, const int64_t *n_dev,
                           int64_t n) {
  return t == n_tiles - 1 ? isect_count(n_dev, n) : (int64_t)offsets[t + 1];
}

struct TileCtx {
  int tile, c, x0, y0;  // flat tile index, its camera, its first pixel
  int64_t start, end;   // its isect range
};

// n_tiles: a.n_tiles, or the product again where the kernel has its factors at
// hand anyway (rasterize.hip: the range's loads then issue among the divisions).
GS_INLINE TileCtx tile_ctx(const TileArgs &a, int tile, int ts, int n_tiles) {
  const int per = a.tw * a.th, c = tile / per, rem = tile - c * per, ty = rem / a.tw;
  return TileCtx{tile, c, (rem - ty * a.tw) * ts, ty * ts, a.offsets[tile],
                 tile_end(a.offsets, tile, n_tiles, nullptr, a.n_isects)};
}

// Pixel p (row-major in the tile of ts x ts) of the tile and its centre; whether
// it lies in the image, and (to be used only there) its index into the [C,H,W]
// images.  p < ts * ts is the caller's to see to.
struct TilePixel {
  int x, y;
  float fx, fy;
};

GS_INLINE TilePixel tile_pixel(const TileCtx &t, int ts, int p) {
  const int ly = p / ts;
  const int x = t.x0 + (p - ly * ts), y = t.y0 + ly;
  return TilePixel{x, y, (float)x + 0.5f, (float)y + 0.5f};
}
GS_INLINE bool in_image(const TileArgs &a, TilePixel px) { return px.x < a.W && px.y < a.H; }
GS_INLINE int64_t image_index(const TileArgs &a, const TileCtx &t, TilePixel px) {
  return ((int64_t)t.c * a.H + px.y) * a.W + px.x;
}

// Geometry of a staged batch of up to B records.
template <int B>
struct Geom {
  float2 xy[B];
  float4 con[B];  // conic a, b, c, opacity
  int32_t gid[B];
};

template <int B>
GS_INLINE void stage_geom(const TileArgs &a, Geom<B> &s, int64_t b0, int nb) {
  const int j = threadIdx.x;
  if (j < nb) {
    const int32_t g = a.flatten_ids[b0 + j];
    s.gid[j] = g;
    s.xy[j] = *reinterpret_cast<const float2 *>(a.means2d + 2 * (int64_t)g);
    const float *cn = a.conics + 3 * (int64_t)g;
    s.con[j] = make_float4(cn[0], cn[1], cn[2], a.opacities[g]);
  }
}

// ---- forward: a record at the pixel centre (fx, fy)
struct FwdRecord {
  float sigma, alpha;
};

GS_INLINE FwdRecord fwd_record(float2 xy, float4 cn, float fx, float fy) {
  const float dx = xy.x - fx, dy = xy.y - fy;
  const float sigma = 0.5f * (cn.x * dx * dx + cn.z * dy * dy) + cn.y * dx * dy;
  return FwdRecord{sigma, fminf(kAlphaMax, cn.w * __expf(-sigma))};
}
GS_INLINE bool blends(const FwdRecord &r) { return r.sigma >= 0.f && r.alpha >= kAlphaMin; }

// ---- backward.  sigma is not the forward's expression: the 0.5 is
// distributed here, and the two round differently.
struct BwdRecord {
  float dx, dy, sigma, ex, alpha_raw;  // ex = exp(-sigma), alpha_raw = opacity * ex
};

GS_INLINE BwdRecord bwd_record(float2 xy, float4 cn, float fx, float fy) {
  const float dx = xy.x - fx, dy = xy.y - fy;
  const float sigma = 0.5f * cn.x * dx * dx + 0.5f * cn.z * dy * dy + cn.y * dx * dy;
  const float ex = __expf(-sigma);
  return BwdRecord{dx, dy, sigma, ex, cn.w * ex};
}
GS_INLINE bool blends(const BwdRecord &r) { return r.sigma >= 0.f && r.alpha_raw >= kAlphaMin; }

// The pixel's gradients of opacity, mean x, y and conic a, b, c from Dalpha,
// the loss gradient of the clamped alpha.
struct GeomGrads {
  float op, mx, my, ca, cb, cc;
};

GS_INLINE GeomGrads geom_grads(float4 cn, const BwdRecord &r, float alpha, float Dalpha) {
  const float aD = alpha * Dalpha;
  return GeomGrads{Dalpha * r.ex, -aD * (cn.x * r.dx + cn.y * r.dy),
                   -aD * (cn.y * r.dx + cn.z * r.dy), -0.5f * aD * r.dx * r.dx,
                   -aD * r.dx * r.dy, -0.5f * aD * r.dy * r.dy};
}

// The largest of the workgroup's my_last (its n_waves <= 4 waves meet in s): the
// backward truncates the tile's range there (rasterize_to_pixels_bwd.py:95-101).
// Holds a __syncthreads().  my_last by reference: by value costs a VGPR.
GS_INLINE int32_t tile_max_last(const int32_t &my_last, int32_t (&s)[4], int n_waves) {
  int32_t wmax = my_last;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) wmax = max(wmax, __shfl_xor(wmax, m, 64));
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = wmax;
  __syncthreads();
  int32_t max_last = s[0];
  for (int w = 1; w < n_waves; ++w) max_last = max(max_last, s[w]);
  return max_last;
}

}  // namespace gs
