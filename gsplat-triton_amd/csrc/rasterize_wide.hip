// Wide-channel tile rasterizer for gfx950: 16x16 tiles, 33..512 colour
// channels (feature fields), the blend on the matrix cores.
//
// rasterize_to_pixels' semantics (rasterize.hip, rasterize16.hip; reference
// rasterize_to_pixels_fwd.py / _bwd.py), with the arithmetic that grows with
// the channel count D taken as matrix products.  With w[p,i] = alpha_i T_i,
// the weight of sorted Gaussian i at pixel p:
//
//   forward   out[P x D]       = w[P x B] colours[B x D]
//   backward  q[B x P]         = colours[B x D] v_out^T[D x P]
//             v_colours[B x D] = w^T[B x P] v_out[P x D]
//
// The alpha walk (conic, exp, transmittance, thresholds, early stop) runs once
// per channel slab on the vector pipe, one lane per pixel, and never touches a
// colour.
//
//   wide_fwd_kernel   workgroup = (tile, slab of 128 channels), 4 waves of 64
//                     pixels.  Per batch of 32 Gaussians: geometry and the
//                     slab's colour rows staged in LDS; each lane walks its
//                     pixel and leaves w in a wave-private LDS row per
//                     Gaussian that any pixel of the wave takes (a ballot;
//                     the others never reach the MFMA); v_mfma_f32_32x32x2_f32
//                     with M = pixels, N = channels, K = a pair of taken
//                     Gaussians into 2 x 4 accumulator tiles that stay in
//                     registers for the whole tile.
//   wide_bwd_kernel   workgroup = (tile, slab of 64 channels), back to front
//                     from T_final.  v_out of the tile is staged in LDS once.
//                     Per batch: q^T by v_mfma_f32_16x16x4_f32 (K = channels)
//                     into LDS [Gaussian][pixel]; the scalar backward per lane
//                     (v_alpha from q, then opacity / conic / mean gradients,
//                     reduce-scattered over the wave, one atomic per field;
//                     the absgrad fields from q over all channels, by slab 0),
//                     which overwrites q with w in place; v_colours by
//                     v_mfma_f32_16x16x4_f32 with K = the tile's 256 pixels,
//                     wave = a block of 16 channels, so a (Gaussian, channel)
//                     sum is complete in one accumulator: one fp32 atomic per
//                     (Gaussian, tile, channel), none for a Gaussian the tile
//                     does not blend.
//
// v_alpha is linear in q, so the slabs add their geometry gradients
// independently; the render-alpha cotangent belongs to slab 0.  Channels past
// D inside the last slab are staged as zeros and never stored.
#include "raster16.h"
#include "wave_ops.h"
#include "../../include/gsplat_hip.h"

namespace gs {
namespace wide {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

using r16::kAlphaMax;
using r16::kAlphaMin;
using r16::kTMin;

constexpr int kMinD = 33, kMaxD = 512;
constexpr int kBatch = 32;     // Gaussians per staged batch
constexpr int kFwdSlab = 128;  // forward: channels per workgroup (4 MFMA column blocks)
constexpr int kBwdSlab = 64;   // backward: channels per workgroup (v_out fits LDS beside w)
// LDS row strides in floats, = 4 mod 64: the 16x16x4 operand reads
// [row = lane % 16][k = lane / 16] then fall on 64 different banks
constexpr int kBwdLd = kBwdSlab + 4;  // v_out [256][.], colours [kBatch][.]
constexpr int kWLd = 256 + 4;         // q / w [kBatch][.]

struct Args {
  int C, D, W, H, tw, th, n_tiles;
  int64_t n_isects;
  const float *means2d, *conics, *colors, *opacities, *backgrounds;  // backgrounds nullable
  const uint8_t *masks;                                              // nullable
  const int32_t *offsets, *flatten_ids;
  float *render_colors, *render_alphas;
  int32_t *last_ids;
  const float *v_render_colors, *v_render_alphas;  // alphas nullable
  float *v_means2d, *v_conics, *v_colors, *v_opacities, *v_abs;  // abs nullable
};

struct Geom {
  float2 xy[kBatch];
  float4 con[kBatch];  // conic a, b, c, opacity
  int32_t gid[kBatch];
};

struct Tile {
  int tile, slab, c, x0, y0;
  int64_t start, end;
};

GS_INLINE Tile tile_of(const Args &a, int nslab) {
  Tile t;
  t.tile = blockIdx.x / nslab;
  t.slab = blockIdx.x - t.tile * nslab;
  const int per = a.tw * a.th;
  t.c = t.tile / per;
  const int rem = t.tile - t.c * per;
  const int ty = rem / a.tw;
  t.x0 = (rem - ty * a.tw) * r16::kTS;
  t.y0 = ty * r16::kTS;
  t.start = a.offsets[t.tile];
  t.end = r16::tile_end(a.offsets, t.tile, a.n_tiles, nullptr, a.n_isects);
  return t;
}

// Pixel p (0..255, row-major in the tile; wave w owns 64 w ..) of the tile:
// its index into the [C,H,W] images, or -1 outside the image.
GS_INLINE int64_t pixel_index(const Args &a, const Tile &t, int p) {
  const int x = t.x0 + (p & 15), y = t.y0 + (p >> 4);
  return (x < a.W && y < a.H) ? ((int64_t)t.c * a.H + y) * a.W + x : -1;
}

GS_INLINE void stage_geom(const Args &a, Geom &s, int64_t b0, int nb) {
  const int j = threadIdx.x;
  if (j < nb) {
    const int32_t g = a.flatten_ids[b0 + j];
    s.gid[j] = g;
    s.xy[j] = *reinterpret_cast<const float2 *>(a.means2d + 2 * (int64_t)g);
    const float *cn = a.conics + 3 * (int64_t)g;
    s.con[j] = make_float4(cn[0], cn[1], cn[2], a.opacities[g]);
  }
}

// Rows b0 .. b0 + nb of the slab's colours into s_col[row][LD]: NC (a power of
// two) columns from channel ch0, zeros past D; with ZERO_ROWS the rows from nb
// to kBatch are zeroed too (they enter a product).
template <int NC, int LD, bool ZERO_ROWS>
GS_INLINE void stage_colors(const Args &a, float *s_col, int64_t b0, int nb, int ch0, int ncols) {
  const int col = threadIdx.x & (NC - 1);
  const int ch = ch0 + col;
  if (col >= ncols) return;
  for (int r = threadIdx.x / NC; r < (ZERO_ROWS ? kBatch : nb); r += 256 / NC) {
    float v = 0.f;
    if (r < nb && ch < a.D) v = a.colors[(int64_t)a.flatten_ids[b0 + r] * a.D + ch];
    s_col[r * LD + col] = v;
  }
}

// ------------------------------------------------------------------ forward
__global__ void __launch_bounds__(256, 2) wide_fwd_kernel(Args a, int nslab) {
  __shared__ Geom s;
  __shared__ float s_col[kBatch * kFwdSlab];
  __shared__ float s_w[4][kBatch * 64];  // per wave: w[Gaussian][pixel]
  __shared__ float s_T[4][64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int i = lane & 31, h = lane >> 5;
  const Tile t = tile_of(a, nslab);
  const int ch0 = t.slab * kFwdSlab;
  const int nblk = min(4, (a.D - ch0 + 31) / 32);  // 32-channel blocks in use
  const int64_t pix = pixel_index(a, t, tid);
  const float fx = (float)(t.x0 + (tid & 15)) + 0.5f, fy = (float)(t.y0 + (tid >> 4)) + 0.5f;

  f32x16 acc[2][4];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mb][nb][r] = 0.f;

  float T = 1.f;
  int32_t last = 0;
  // masks[tile] != 0 skips the tile: its pixels are written as background
  const bool skip_tile = a.masks && a.masks[t.tile];
  bool done = pix < 0 || skip_tile;
  float *wl = s_w[wid];

  if (!skip_tile) {
    for (int64_t b0 = t.start; b0 < t.end; b0 += kBatch) {
      // every pixel terminated: the tile stops (also the LDS WAR fence)
      if (__syncthreads_count(!done) == 0) break;
      const int nb = (int)min((int64_t)kBatch, t.end - b0);
      stage_geom(a, s, b0, nb);
      stage_colors<kFwdSlab, kFwdSlab, false>(a, s_col, b0, nb, ch0, 32 * nblk);
      __syncthreads();

      // the walk: bit k of `taken` = some pixel of the wave blends Gaussian k
      uint32_t taken = 0;
      if (__ballot(!done) != 0) {
        for (int k = 0; k < nb; ++k) {
          float w = 0.f;
          if (!done) {
            const float2 xy = s.xy[k];
            const float4 cn = s.con[k];
            const float dx = xy.x - fx, dy = xy.y - fy;
            const float sigma = 0.5f * (cn.x * dx * dx + cn.z * dy * dy) + cn.y * dx * dy;
            const float alpha = fminf(kAlphaMax, cn.w * __expf(-sigma));
            if (sigma >= 0.f && alpha >= kAlphaMin) {
              const float next_T = T * (1.f - alpha);
              if (next_T <= kTMin) {
                done = true;
              } else {
                w = alpha * T;
                T = next_T;
                last = (int32_t)(b0 + k);
              }
            }
          }
          if (__ballot(w != 0.f) != 0) {
            wl[k * 64 + lane] = w;
            taken |= 1u << k;
          }
        }
      }
      wave_sync_lds();

      // the blend: pairs of taken Gaussians are the K = 2 of one MFMA step;
      // lane half h carries Gaussian h of the pair, an odd tail a zero weight
      taken = __builtin_amdgcn_readfirstlane(taken);
      while (taken) {
        const int k0 = __builtin_ctz(taken);
        taken &= taken - 1;
        const bool pair = taken != 0;
        const int k1 = pair ? __builtin_ctz(taken) : k0;
        if (pair) taken &= taken - 1;
        const int k = h ? k1 : k0;
        const bool pad = h && !pair;
        const float a0 = pad ? 0.f : wl[k * 64 + i];
        const float a1 = pad ? 0.f : wl[k * 64 + 32 + i];
#pragma unroll
        for (int nb4 = 0; nb4 < 4; ++nb4)
          if (nb4 < nblk) {
            const float b = s_col[k * kFwdSlab + 32 * nb4 + i];
            acc[0][nb4] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc[0][nb4], 0, 0, 0);
            acc[1][nb4] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc[1][nb4], 0, 0, 0);
          }
      }
    }
  }

  if (t.slab == 0 && pix >= 0) {
    a.render_alphas[pix] = 1.f - T;
    a.last_ids[pix] = last;
  }
  // accumulator register r of lane half h holds pixel row (r & 3) + 8 (r >> 2)
  // + 4 h of its 32-pixel block, column = channel i of the 32-channel block
  s_T[wid][lane] = T;
  wave_sync_lds();
  float bg[4];
#pragma unroll
  for (int nb4 = 0; nb4 < 4; ++nb4) {
    const int ch = ch0 + 32 * nb4 + i;
    bg[nb4] = (a.backgrounds && ch < a.D) ? a.backgrounds[(int64_t)t.c * a.D + ch] : 0.f;
  }
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int p = 32 * mb + (r & 3) + 8 * (r >> 2) + 4 * h;
      const int64_t px = pixel_index(a, t, 64 * wid + p);
      if (px < 0) continue;
      const float Tp = s_T[wid][p];
      float *out = a.render_colors + px * a.D;
#pragma unroll
      for (int nb4 = 0; nb4 < 4; ++nb4) {
        const int ch = ch0 + 32 * nb4 + i;
        if (nb4 < nblk && ch < a.D) out[ch] = acc[mb][nb4][r] + Tp * bg[nb4];
      }
    }
}

// ----------------------------------------------------------------- backward
template <bool ABS>
__global__ void __launch_bounds__(256) wide_bwd_kernel(Args a, int nslab) {
  __shared__ Geom s;
  __shared__ float s_vout[256 * kBwdLd];  // v_out[pixel][channel] of the tile and slab
  __shared__ float s_col[kBatch * kBwdLd];
  __shared__ float s_qw[kBatch * kWLd];  // q, then w, [Gaussian][pixel]
  __shared__ float s_qa[ABS ? kBatch * kWLd : 1];  // q over all channels (see `multi`)
  __shared__ int32_t s_maxlast[4];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int i = lane & 15, j = lane >> 4;
  const Tile t = tile_of(a, nslab);
  if (a.masks && a.masks[t.tile]) return;
  const int ch0 = t.slab * kBwdSlab;
  const int nch = min(kBwdSlab, a.D - ch0);
  const int ksteps = (nch + 3) / 4;
  const int64_t pix = pixel_index(a, t, tid);
  const float fx = (float)(t.x0 + (tid & 15)) + 0.5f, fy = (float)(t.y0 + (tid >> 4)) + 0.5f;

  // v_out of the tile, zeros outside the image and past D
  {
    const int col = tid & (kBwdSlab - 1);
    const bool live = ch0 + col < a.D;
    for (int p = tid / kBwdSlab; p < 256; p += 256 / kBwdSlab) {
      const int64_t px = pixel_index(a, t, p);
      s_vout[p * kBwdLd + col] =
          (live && px >= 0) ? a.v_render_colors[px * a.D + ch0 + col] : 0.f;
    }
  }

  float T_final = 1.f, Dra = 0.f;
  int32_t my_last = -1;
  if (pix >= 0) {
    T_final = 1.f - a.render_alphas[pix];
    if (t.slab == 0 && a.v_render_alphas) Dra = a.v_render_alphas[pix];
    my_last = a.last_ids[pix];
  }
  // truncate the tile's range at the last contributor of any pixel
  int32_t wmax = my_last;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) wmax = max(wmax, __shfl_xor(wmax, m, 64));
  if (lane == 0) s_maxlast[wid] = wmax;
  __syncthreads();
  const int32_t max_last = max(max(s_maxlast[0], s_maxlast[1]), max(s_maxlast[2], s_maxlast[3]));
  const int64_t end = min(t.end, (int64_t)max_last + 1);

  // T_final (v_render_alpha - bg . v_out), this slab's share
  float fin = T_final * Dra;
  if (a.backgrounds) {
    float dot = 0.f;
    for (int c = 0; c < nch; ++c)
      dot += a.backgrounds[(int64_t)t.c * a.D + ch0 + c] * s_vout[tid * kBwdLd + c];
    fin -= T_final * dot;
  }

  // |v_means2d| is not linear in q: it needs the pixel's whole v_alpha.  With
  // more than one slab, slab 0 also forms q over all channels (the operands of
  // the further slabs straight from global memory) and owns the abs fields.
  const bool multi = ABS && nslab > 1 && t.slab == 0;
  float fin_a = fin;
  int64_t pxs[4];
#pragma unroll
  for (int pb = 0; pb < 4; ++pb) pxs[pb] = pixel_index(a, t, 64 * wid + 16 * pb + i);
  if (multi && pix >= 0 && a.backgrounds) {
    float dot = 0.f;
    for (int c = 0; c < a.D; ++c)
      dot += a.backgrounds[(int64_t)t.c * a.D + c] * a.v_render_colors[pix * a.D + c];
    fin_a = T_final * (Dra - dot);
  }

  float T = T_final;  // exclusive transmittance of the Gaussian being visited
  float rD = 0.f;     // sum over the visited Gaussians of w q
  float rD_a = 0.f;   // the same with q over all channels
  constexpr int NF = ABS ? 8 : 6;
  const int lf = rs_field(lane);

  for (int64_t b1 = end; b1 > t.start; b1 -= kBatch) {
    const int64_t b0 = max(t.start, b1 - kBatch);
    const int nb = (int)(b1 - b0);
    __syncthreads();  // the previous batch is consumed
    stage_geom(a, s, b0, nb);
    stage_colors<kBwdSlab, kBwdLd, true>(a, s_col, b0, nb, ch0, kBwdSlab);
    __syncthreads();

    // 1. q^T[Gaussian][pixel] = colours v_out^T for the wave's 64 pixels:
    // A = colours[g = 16 gb + i][ch = 4 st + j], B = v_out[pixel = 16 pb + i][ch]
    {
      f32x4 q[4][2];
#pragma unroll
      for (int pb = 0; pb < 4; ++pb)
#pragma unroll
        for (int gb = 0; gb < 2; ++gb) q[pb][gb] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int st = 0; st < ksteps; ++st) {
        const int ch = 4 * st + j;
        const float c0 = s_col[i * kBwdLd + ch], c1 = s_col[(16 + i) * kBwdLd + ch];
#pragma unroll
        for (int pb = 0; pb < 4; ++pb) {
          const float v = s_vout[(64 * wid + 16 * pb + i) * kBwdLd + ch];
          q[pb][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(c0, v, q[pb][0], 0, 0, 0);
          q[pb][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(c1, v, q[pb][1], 0, 0, 0);
        }
      }
      // register r of lane (i, j) holds row 4 j + r (Gaussian), column i (pixel)
#pragma unroll
      for (int pb = 0; pb < 4; ++pb)
#pragma unroll
        for (int gb = 0; gb < 2; ++gb)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            s_qw[(16 * gb + 4 * j + r) * kWLd + 64 * wid + 16 * pb + i] = q[pb][gb][r];
      if (multi) {
        const int64_t g0 = i < nb ? (int64_t)s.gid[i] * a.D : -1;
        const int64_t g1 = 16 + i < nb ? (int64_t)s.gid[16 + i] * a.D : -1;
        for (int c4 = kBwdSlab; c4 < a.D; c4 += 4) {
          const int ch = c4 + j;
          const bool live = ch < a.D;
          const float c0 = (live && g0 >= 0) ? a.colors[g0 + ch] : 0.f;
          const float c1 = (live && g1 >= 0) ? a.colors[g1 + ch] : 0.f;
#pragma unroll
          for (int pb = 0; pb < 4; ++pb) {
            const float v = (live && pxs[pb] >= 0) ? a.v_render_colors[pxs[pb] * a.D + ch] : 0.f;
            q[pb][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(c0, v, q[pb][0], 0, 0, 0);
            q[pb][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(c1, v, q[pb][1], 0, 0, 0);
          }
        }
#pragma unroll
        for (int pb = 0; pb < 4; ++pb)
#pragma unroll
          for (int gb = 0; gb < 2; ++gb)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              s_qa[(16 * gb + 4 * j + r) * kWLd + 64 * wid + 16 * pb + i] = q[pb][gb][r];
      }
    }
    wave_sync_lds();  // a wave reads back its own 64 columns only

    // 2. the scalar backward, lane = pixel; q[k][pixel] becomes w[k][pixel]
    for (int k = nb - 1; k >= 0; --k) {
      const int64_t idx = b0 + k;
      const float2 xy = s.xy[k];
      const float4 cn = s.con[k];
      const float dx = xy.x - fx, dy = xy.y - fy;
      const float sigma = 0.5f * cn.x * dx * dx + 0.5f * cn.z * dy * dy + cn.y * dx * dy;
      const float ex = __expf(-sigma);
      const float alpha_raw = cn.w * ex;
      const bool valid = (idx <= my_last) && (sigma >= 0.f) && (alpha_raw >= kAlphaMin);
      float w = 0.f;
      if (__ballot(valid) != 0) {
        float g[NF];
#pragma unroll
        for (int f = 0; f < NF; ++f) g[f] = 0.f;
        if (valid) {
          const float alpha = fminf(kAlphaMax, alpha_raw);
          const float ra = 1.f / (1.f - alpha);
          T *= ra;
          w = alpha * T;
          const float q = s_qw[k * kWLd + tid];
          rD += q * w;
          float Dalpha = ra * (fin + T * q - rD);
          if (alpha_raw > kAlphaMax) Dalpha = 0.f;  // a clamped alpha has no gradient
          const float aD = alpha * Dalpha;
          g[0] = Dalpha * ex;
          g[1] = -aD * (cn.x * dx + cn.y * dy);
          g[2] = -aD * (cn.y * dx + cn.z * dy);
          g[3] = -0.5f * aD * dx * dx;
          g[4] = -aD * dx * dy;
          g[5] = -0.5f * aD * dy * dy;
          if constexpr (ABS) {
            if (t.slab == 0) {
              const float qa = multi ? s_qa[k * kWLd + tid] : q;
              rD_a += qa * w;
              float Da = ra * (fin_a + T * qa - rD_a);
              if (alpha_raw > kAlphaMax) Da = 0.f;
              const float aDa = alpha * Da;
              g[6] = fabsf(aDa * (cn.x * dx + cn.y * dy));
              g[7] = fabsf(aDa * (cn.y * dx + cn.z * dy));
            }
          }
        }
        const float tot = reduce_scatter<NF>(g, lane);
        if ((lane & 3) == 0 && lf < NF && tot != 0.f) {
          const int64_t gi = s.gid[k];
          float *dst = lf == 0 ? a.v_opacities + gi
                     : lf < 3  ? a.v_means2d + 2 * gi + (lf - 1)
                     : lf < 6  ? a.v_conics + 3 * gi + (lf - 3)
                               : a.v_abs + 2 * gi + (lf - 6);
          atomic_add_f32(dst, tot);
        }
      }
      s_qw[k * kWLd + tid] = w;
    }
    __syncthreads();

    // 3. v_colours[Gaussian][channel] = w^T v_out over the tile's 256 pixels;
    // wave = channels 16 wid ..: A = w[g = 16 gb + i][pixel = 4 st + j],
    // B = v_out[pixel][ch = 16 wid + i].  Rows past nb hold w = 0.
    if (16 * wid < nch) {
      f32x4 vc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll 4
      for (int st = 0; st < 64; ++st) {
        const int p = 4 * st + j;
        const float v = s_vout[p * kBwdLd + 16 * wid + i];
        vc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(s_qw[i * kWLd + p], v, vc[0], 0, 0, 0);
        vc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(s_qw[(16 + i) * kWLd + p], v, vc[1], 0, 0, 0);
      }
      const int ch = ch0 + 16 * wid + i;
#pragma unroll
      for (int gb = 0; gb < 2; ++gb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * gb + 4 * j + r;
          const float v = vc[gb][r];
          if (row < nb && ch < a.D && v != 0.f)
            atomic_add_f32(a.v_colors + (int64_t)s.gid[row] * a.D + ch, v);
        }
    }
  }
}

static int check(const char *who, int C, int D, int W, int H, int ts, int tw, int th,
                 int64_t n_isects) {
  GS_REQUIRE(ts == r16::kTS, "%s: tile_size %d is not supported (16 only)", who, ts);
  GS_REQUIRE(D >= kMinD && D <= kMaxD, "%s: %d channels not in [%d, %d]", who, D, kMinD, kMaxD);
  GS_REQUIRE(C >= 0 && W >= 0 && H >= 0 && n_isects >= 0, "%s: negative sizes", who);
  GS_REQUIRE((int64_t)tw * ts >= W && (int64_t)th * ts >= H,
             "%s: tile grid %dx%d x %d does not cover %dx%d", who, tw, th, ts, W, H);
  GS_REQUIRE((int64_t)C * tw * th * ((kMaxD + kBwdSlab - 1) / kBwdSlab) < (1ll << 31),
             "%s: too many tiles", who);
  return 0;
}

}  // namespace wide
}  // namespace gs

using namespace gs;

extern "C" int gsplat_hip_rasterize_wide_supported(int D, int tile_size) {
  return tile_size == r16::kTS && D >= wide::kMinD && D <= wide::kMaxD;
}

extern "C" int gsplat_hip_rasterize_wide_fwd(
    int C, int D, int width, int height, int tile_size, int tile_width, int tile_height,
    const float *means2d, const float *conics, const float *colors, const float *opacities,
    const float *backgrounds, const uint8_t *masks, const int32_t *isect_offsets,
    int64_t n_isects, const int32_t *flatten_ids, float *render_colors, float *render_alphas,
    int32_t *last_ids, void *stream) {
  if (int e = wide::check("rasterize_wide_fwd", C, D, width, height, tile_size, tile_width,
                          tile_height, n_isects))
    return e;
  wide::Args a{};
  a.C = C; a.D = D; a.W = width; a.H = height; a.tw = tile_width; a.th = tile_height;
  a.n_tiles = C * tile_width * tile_height;
  if (a.n_tiles == 0) return 0;
  a.n_isects = n_isects;
  a.means2d = means2d; a.conics = conics; a.colors = colors; a.opacities = opacities;
  a.backgrounds = backgrounds; a.masks = masks; a.offsets = isect_offsets;
  a.flatten_ids = flatten_ids;
  a.render_colors = render_colors; a.render_alphas = render_alphas; a.last_ids = last_ids;
  const int nslab = (D + wide::kFwdSlab - 1) / wide::kFwdSlab;
  hipLaunchKernelGGL(wide::wide_fwd_kernel, dim3((unsigned)(a.n_tiles * nslab)), dim3(256), 0,
                     (hipStream_t)stream, a, nslab);
  GS_CHECK_LAUNCH("rasterize_wide_fwd");
  return 0;
}

// The gradient buffers are zeroed here (on `stream`) before accumulation.
extern "C" int gsplat_hip_rasterize_wide_bwd(
    int C, int64_t n_gaussians, int D, int width, int height, int tile_size, int tile_width,
    int tile_height, const float *means2d, const float *conics, const float *colors,
    const float *opacities, const float *backgrounds, const uint8_t *masks,
    const int32_t *isect_offsets, int64_t n_isects, const int32_t *flatten_ids,
    const float *render_alphas, const int32_t *last_ids, const float *v_render_colors,
    const float *v_render_alphas, float *v_means2d, float *v_conics, float *v_colors,
    float *v_opacities, float *v_means2d_abs, void *stream) {
  if (int e = wide::check("rasterize_wide_bwd", C, D, width, height, tile_size, tile_width,
                          tile_height, n_isects))
    return e;
  GS_REQUIRE(n_gaussians >= 0, "rasterize_wide_bwd: negative sizes");
  hipStream_t st = (hipStream_t)stream;
  const size_t G = (size_t)n_gaussians;
  GS_HIP(gs::zero_async(v_means2d, sizeof(float) * 2 * G, st));
  GS_HIP(gs::zero_async(v_conics, sizeof(float) * 3 * G, st));
  GS_HIP(gs::zero_async(v_colors, sizeof(float) * D * G, st));
  GS_HIP(gs::zero_async(v_opacities, sizeof(float) * G, st));
  if (v_means2d_abs) GS_HIP(gs::zero_async(v_means2d_abs, sizeof(float) * 2 * G, st));
  wide::Args a{};
  a.C = C; a.D = D; a.W = width; a.H = height; a.tw = tile_width; a.th = tile_height;
  a.n_tiles = C * tile_width * tile_height;
  if (a.n_tiles == 0 || n_isects == 0) return 0;
  a.n_isects = n_isects;
  a.means2d = means2d; a.conics = conics; a.colors = colors; a.opacities = opacities;
  a.backgrounds = backgrounds; a.masks = masks; a.offsets = isect_offsets;
  a.flatten_ids = flatten_ids;
  a.render_alphas = const_cast<float *>(render_alphas);
  a.last_ids = const_cast<int32_t *>(last_ids);
  a.v_render_colors = v_render_colors; a.v_render_alphas = v_render_alphas;
  a.v_means2d = v_means2d; a.v_conics = v_conics; a.v_colors = v_colors;
  a.v_opacities = v_opacities; a.v_abs = v_means2d_abs;
  const int nslab = (D + wide::kBwdSlab - 1) / wide::kBwdSlab;
  const dim3 grid((unsigned)(a.n_tiles * nslab));
  if (v_means2d_abs)
    hipLaunchKernelGGL(wide::wide_bwd_kernel<true>, grid, dim3(256), 0, st, a, nslab);
  else
    hipLaunchKernelGGL(wide::wide_bwd_kernel<false>, grid, dim3(256), 0, st, a, nslab);
  GS_CHECK_LAUNCH("rasterize_wide_bwd");
  return 0;
}
