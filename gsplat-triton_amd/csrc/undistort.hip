// Image undistortion for gfx950: uint8 source images -> float32 undistorted
// images, the device counterpart of cv2.remap(image, mapx, mapy, INTER_LINEAR)
// with a constant 0 border followed by the ROI crop
// (examples/datasets/colmap.py:258-325, 366-374).
//
//   gsplat_hip_undistort_u8_f32   the source coordinate of every output pixel
//                                 is evaluated in the kernel (no map tables in
//                                 memory): OpenCV's initUndistortRectifyMap
//                                 with R = I (model 0) or the reference's
//                                 fisheye formula (model 1)
//   gsplat_hip_remap_u8_f32       the same remap from explicit mapx / mapy
//
// One templated body.  A block owns 256 consecutive output pixels of the
// flattened [h, w] output, one lane per pixel.  The lane evaluates its source
// coordinate once (float64, rounded to float32 as OpenCV stores its maps), the
// offsets of its two pairs of horizontal neighbours and the four fp32 weights,
// and then walks the B images that share the map: two 12-B loads (load_pair:
// the 6 bytes of a pair inside three aligned dwords; 12 single byte loads
// measured 0.69 ms where this takes 0.40-0.44 ms, 8 images of 4000x3000), three
// blends, three floats into an LDS tile (two tiles take turns, the next
// image's bytes are requested before the barrier).  The tile (768 floats, contiguous in the output) is then stored
// by the block as 16-B vectors: a pixel is 12 B, so a lane storing its own
// pixel would issue three 4-B stores at a 12-B stride.  Rows of 3 w floats
// and images of 3 h w floats are not multiples of 16 B, so the first store
// address of a block is 16-B aligned only by luck: up to three leading and
// three trailing floats of the tile go out as single floats, the rest as
// aligned float4.  No atomics: every output float is written once, by one
// lane, from values that do not depend on the launch.
//
// Bytes per output pixel and image: 3 read (each source byte is used by the
// four output pixels around it, from the caches), 12 written.
#include "common.h"
#include "../../include/gsplat_hip.h"

namespace gs {
namespace ud {

enum { kPerspective = 0, kFisheye = 1 };
constexpr int kBlock = 256;

struct Args {
  int B, H, W;  // source images [B, H, W, 3]
  int h, w;     // output images [B, h, w, 3]
  int rx, ry;   // ROI origin: output pixel (u, v) is pixel (u + rx, v + ry) of the full frame
  int model;
  double fx, fy, cx, cy;      // K of the distorted camera
  double k[4];                // k1 k2 p1 p2 (perspective), k1 k2 k3 k4 (fisheye)
  double nfx, nfy, ncx, ncy;  // K of the undistorted full frame
  float scale;
  const uint8_t *src;
  float *out;
  const float *mapx, *mapy;  // [h, w], table form only
};

// The map in float64 without contraction, as numpy evaluates the host maps
// (colmap.undistort_maps), rounded to float32 at the end.
GS_INLINE void eval_map(const Args &a, int u, int v, float &sx, float &sy) {
#pragma clang fp contract(off)
  const double x = ((double)(u + a.rx) - a.ncx) / a.nfx;
  const double y = ((double)(v + a.ry) - a.ncy) / a.nfy;
  const double r2 = x * x + y * y;
  if (a.model == kPerspective) {
    const double kr = 1.0 + (a.k[1] * r2 + a.k[0]) * r2;
    const double xy = x * y;
    const double xd = x * kr + 2.0 * a.k[2] * xy + a.k[3] * (r2 + 2.0 * (x * x));
    const double yd = y * kr + a.k[2] * (r2 + 2.0 * (y * y)) + 2.0 * a.k[3] * xy;
    sx = (float)(a.fx * xd + a.cx);
    sy = (float)(a.fy * yd + a.cy);
  } else {
    const double r4 = r2 * r2;
    const double r = 1.0 + a.k[0] * r2 + a.k[1] * r4 + a.k[2] * (r4 * r2) + a.k[3] * (r4 * r4);
    sx = (float)(a.fx * x * r + (double)(a.W / 2));
    sy = (float)(a.fy * y * r + (double)(a.H / 2));
  }
}

// Six consecutive bytes from any address as three aligned dwords (one 12-B
// load) and a byte offset `sh` into them, instead of six byte loads.  The
// dwords start at the dword that holds `p[0]`, or earlier where that would
// run past the dword holding the last byte of the source buffer (`end[-1]`):
// then `sh` grows up to 11 and the bytes past the 12 read count as 0 (they lie
// outside the buffer, where every neighbour weighs 0).  A dword lies in one
// page, so no read leaves the pages of the buffer.  WIDE needs a buffer of 16
// bytes or more; smaller ones are read byte by byte.
typedef uint32_t __attribute__((may_alias)) u32a;

struct Raw {
  uint32_t d0, d1, d2, sh;
};

template <bool WIDE>
GS_INLINE Raw load_pair(const uint8_t *p, const uint8_t *end) {
  Raw r;
  if (WIDE) {
    const uint8_t *q = p - ((uintptr_t)p & 3);
    const uint8_t *last = end + ((4 - ((uintptr_t)end & 3)) & 3) - 12;
    const uint8_t *qa = q < last ? q : last;
    const u32a *d = reinterpret_cast<const u32a *>(qa);
    r.d0 = d[0];
    r.d1 = d[1];
    r.d2 = d[2];
    r.sh = (uint32_t)(p - qa);
  } else {
    uint32_t v[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) v[i] = p + i < end ? (uint32_t)p[i] : 0u;
    r.d0 = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
    r.d1 = v[4] | (v[5] << 8);
    r.d2 = 0u;
    r.sh = 0u;
  }
  return r;
}

// f[0..2]: the first pixel's channels, f[3..5]: the second pixel's.
GS_INLINE void unpack_pair(const Raw &r, float (&f)[6]) {
  const uint32_t k = r.sh >> 2, s = (r.sh & 3u) * 8u;
  const uint32_t e0 = k == 0 ? r.d0 : (k == 1 ? r.d1 : r.d2);
  const uint32_t e1 = k == 0 ? r.d1 : (k == 1 ? r.d2 : 0u);
  const uint32_t e2 = k == 0 ? r.d2 : 0u;
  const uint32_t lo = (uint32_t)(((((uint64_t)e1) << 32) | e0) >> s);
  const uint32_t hi = (uint32_t)(((((uint64_t)e2) << 32) | e1) >> s);
  f[0] = (float)(lo & 255u);
  f[1] = (float)((lo >> 8) & 255u);
  f[2] = (float)((lo >> 16) & 255u);
  f[3] = (float)(lo >> 24);
  f[4] = (float)(hi & 255u);
  f[5] = (float)((hi >> 8) & 255u);
}

template <bool TABLE, bool WIDE>
__global__ void __launch_bounds__(kBlock) undistort_kernel(Args a) {
  __shared__ float tiles[2][3 * kBlock];
  const uint32_t npix = (uint32_t)a.h * (uint32_t)a.w;
  const uint32_t p0 = blockIdx.x * (uint32_t)kBlock;
  const uint32_t p = p0 + threadIdx.x;
  const bool in = p < npix;

  float sx = 0.f, sy = 0.f;
  if (in) {
    if (TABLE) {
      sx = a.mapx[p];
      sy = a.mapy[p];
    } else {
      const uint32_t v = p / (uint32_t)a.w;
      eval_map(a, (int)(p - v * (uint32_t)a.w), (int)v, sx, sy);
    }
  }
  // Neighbours (x0, y0) .. (x0 + 1, y0 + 1), read as two pairs of horizontal
  // neighbours: 6 consecutive bytes each.  A pair starts at column
  // max(x0, 0) of row y0 or y0 + 1 clamped into the image; a neighbour
  // outside the source keeps weight 0 and its place is taken by a byte that
  // is there.  The range test comes first, in float: it is false for NaN and
  // keeps the float -> int conversion in range.
  const bool near = in && sx > -1.f && sx < (float)a.W && sy > -1.f && sy < (float)a.H;
  float wTL = 0.f, wTR = 0.f, wBL = 0.f, wBR = 0.f;
  int oT = 0, oB = 0;
  if (near) {
    const float x0f = floorf(sx), y0f = floorf(sy);
    const float wx = sx - x0f, wy = sy - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;  // -1 <= x0 <= W - 1, -1 <= y0 <= H - 1
    // column weights of the pair's samples xs, xs + 1
    const int xs = max(x0, 0);
    const float cl = x0 < 0 ? wx : 1.f - wx;
    const float cr = (x0 >= 0 && x0 + 1 < a.W) ? wx : 0.f;
    // rows yt (weight rt) and yb (weight rb)
    const int yt = max(y0, 0);
    const int yb = min(y0 + 1, a.H - 1);
    const float rt = y0 < 0 ? 0.f : 1.f - wy;
    const float rb = y0 + 1 < a.H ? wy : 0.f;
    wTL = cl * rt; wTR = cr * rt;
    wBL = cl * rb; wBR = cr * rb;
    oT = (yt * a.W + xs) * 3;
    oB = (yb * a.W + xs) * 3;
  }

  const size_t src_stride = (size_t)a.H * a.W * 3;
  const uint8_t *src_end = a.src + (size_t)a.B * src_stride;
  const int nfl = 3 * (int)min((uint32_t)kBlock, npix - p0);  // this block's floats per image
  // The bytes of image b + 1 are requested before the barrier of image b and
  // unpacked after it, so they are in flight while the tile of image b is
  // stored; two tiles taking turns need one barrier per image (a lane can be
  // one image ahead of the slowest lane of its block, never two).
  Raw rawT = load_pair<WIDE>(a.src + oT, src_end), rawB = load_pair<WIDE>(a.src + oB, src_end);
  for (int b = 0; b < a.B; ++b) {
    float *tile = tiles[b & 1];
    float pT[6], pB[6];
    unpack_pair(rawT, pT);
    unpack_pair(rawB, pB);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float top = wTL * pT[c] + wTR * pT[3 + c];
      const float bot = wBL * pB[c] + wBR * pB[3 + c];
      tile[3 * threadIdx.x + c] = (top + bot) * a.scale;
    }
    if (b + 1 < a.B) {
      const uint8_t *s = a.src + (size_t)(b + 1) * src_stride;
      rawT = load_pair<WIDE>(s + oT, src_end);
      rawB = load_pair<WIDE>(s + oB, src_end);
    }
    __syncthreads();
    float *dst = a.out + ((size_t)b * npix + p0) * 3;
    const int lead = min((int)((4u - (uint32_t)(((uintptr_t)dst >> 2) & 3u)) & 3u), nfl);
    const int nvec = (nfl - lead) >> 2;
    const int t = (int)threadIdx.x;
    if (t < nvec) {
      const int i = lead + 4 * t;
      *reinterpret_cast<float4 *>(dst + i) =
          make_float4(tile[i], tile[i + 1], tile[i + 2], tile[i + 3]);
    }
    if (t < lead) dst[t] = tile[t];
    const int t0 = lead + 4 * nvec;
    if (t0 + t < nfl) dst[t0 + t] = tile[t0 + t];
  }
}

static int launch(const char *name, bool table, const Args &a, hipStream_t st) {
  GS_REQUIRE(a.B >= 0 && a.H >= 0 && a.W >= 0 && a.h >= 0 && a.w >= 0,
             "%s: negative sizes B=%d H=%d W=%d h=%d w=%d", name, a.B, a.H, a.W, a.h, a.w);
  if (a.B == 0 || a.h == 0 || a.w == 0) return 0;
  GS_REQUIRE(a.H > 0 && a.W > 0, "%s: empty source images (H=%d W=%d)", name, a.H, a.W);
  GS_REQUIRE((int64_t)a.H * a.W * 3 < ((int64_t)1 << 31) && (int64_t)a.h * a.w * 3 < ((int64_t)1 << 31),
             "%s: an image of 2^31 bytes or floats and more (H=%d W=%d h=%d w=%d)", name, a.H,
             a.W, a.h, a.w);
  GS_REQUIRE(a.src && a.out, "%s: null pointer argument", name);
  GS_REQUIRE(((uintptr_t)a.out & 3) == 0, "%s: out must be 4-B aligned", name);
  const unsigned blocks = (unsigned)(((int64_t)a.h * a.w + kBlock - 1) / kBlock);
  const bool wide = (int64_t)a.B * a.H * a.W * 3 >= 16;  // load_pair's 12-B reads fit
  auto k = table ? (wide ? undistort_kernel<true, true> : undistort_kernel<true, false>)
                 : (wide ? undistort_kernel<false, true> : undistort_kernel<false, false>);
  hipLaunchKernelGGL(k, dim3(blocks), dim3(kBlock), 0, st, a);
  return 0;
}

}  // namespace ud
}  // namespace gs

using namespace gs;

extern "C" int gsplat_hip_undistort_u8_f32(int B, int H, int W, const uint8_t *images, double fx,
                                           double fy, double cx, double cy, double k1, double k2,
                                           double k3, double k4, double new_fx, double new_fy,
                                           double new_cx, double new_cy, int roi_x, int roi_y,
                                           int w, int h, int model, float scale, float *out,
                                           void *stream) {
  GS_REQUIRE(model == ud::kPerspective || model == ud::kFisheye,
             "undistort_u8_f32: model %d (0 perspective, 1 fisheye)", model);
  GS_REQUIRE(fx != 0.0 && fy != 0.0 && new_fx != 0.0 && new_fy != 0.0,
             "undistort_u8_f32: a focal length is zero");
  // the full-frame pixel u + roi_x is formed in int
  GS_REQUIRE(roi_x > -(1 << 30) && roi_x < (1 << 30) && roi_y > -(1 << 30) && roi_y < (1 << 30),
             "undistort_u8_f32: ROI origin (%d, %d) out of range", roi_x, roi_y);
  ud::Args a{B, H, W, h, w, roi_x, roi_y, model, fx, fy, cx, cy, {k1, k2, k3, k4},
             new_fx, new_fy, new_cx, new_cy, scale, images, out, nullptr, nullptr};
  const int rc = ud::launch("undistort_u8_f32", false, a, (hipStream_t)stream);
  if (rc) return rc;
  GS_CHECK_LAUNCH("undistort_u8_f32");
  return 0;
}

extern "C" int gsplat_hip_remap_u8_f32(int B, int H, int W, const uint8_t *images,
                                       const float *mapx, const float *mapy, int w, int h,
                                       float scale, float *out, void *stream) {
  ud::Args a{B, H, W, h, w, 0, 0, 0, 1.0, 1.0, 0.0, 0.0, {0.0, 0.0, 0.0, 0.0},
             1.0, 1.0, 0.0, 0.0, scale, images, out, mapx, mapy};
  GS_REQUIRE(B <= 0 || h <= 0 || w <= 0 || (mapx && mapy), "remap_u8_f32: null map");
  const int rc = ud::launch("remap_u8_f32", true, a, (hipStream_t)stream);
  if (rc) return rc;
  GS_CHECK_LAUNCH("remap_u8_f32");
  return 0;
}
