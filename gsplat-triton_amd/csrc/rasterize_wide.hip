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
//
// The argument block, the tile and pixel walk, the geometry staging and the
// per-record alpha steps are raster_tile.h's, shared with rasterize.hip.
#include "raster16.h"
#include "wave_ops.h"
#include "../../include/gsplat_hip.h"

namespace gs {
namespace wide {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMinD = 33, kMaxD = 512;
constexpr int kBatch = 32;     // Gaussians per staged batch
constexpr int kFwdSlab = 128;  // forward: channels per workgroup (4 MFMA column blocks)
constexpr int kBwdSlab = 64;   // backward: channels per workgroup (v_out fits LDS beside w)
// LDS row strides in floats, = 4 mod 64: the 16x16x4 operand reads
// [row = lane % 16][k = lane / 16] then fall on 64 different banks
constexpr int kBwdLd = kBwdSlab + 4;  // v_out [256][.], colours [kBatch][.]
constexpr int kWLd = 256 + 4;         // q / w [kBatch][.]

// Pixel p (0..255, row-major in the tile; wave w owns 64 w ..) of the tile:
// its index into the [C,H,W] images, or -1 outside the image.
GS_INLINE int64_t pixel_index(const TileArgs &a, const TileCtx &t, int p) {
  const TilePixel px = tile_pixel(t, r16::kTS, p);
  return in_image(a, px) ? image_index(a, t, px) : -1;
}

// Rows b0 .. b0 + nb of the slab's colours into s_col[row][LD]: NC (a power of
// two) columns from channel ch0, zeros past D; with ZERO_ROWS the rows from nb
// to kBatch are zeroed too (they enter a product).
template <int NC, int LD, bool ZERO_ROWS>
GS_INLINE void stage_colors(const TileArgs &a, float *s_col, int64_t b0, int nb, int ch0,
                            int ncols) {
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
__global__ void __launch_bounds__(256, 2) wide_fwd_kernel(TileArgs a, int nslab) {
  __shared__ Geom<kBatch> s;
  __shared__ float s_col[kBatch * kFwdSlab];
  __shared__ float s_w[4][kBatch * 64];  // per wave: w[Gaussian][pixel]
  __shared__ float s_T[4][64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int i = lane & 31, h = lane >> 5;
  // workgroup = (tile, slab): blockIdx.x = tile * nslab + slab
  const int tile = blockIdx.x / nslab, slab = blockIdx.x - tile * nslab;
  const TileCtx t = tile_ctx(a, tile, r16::kTS, a.n_tiles);
  const int ch0 = slab * kFwdSlab;
  const int nblk = min(4, (a.D - ch0 + 31) / 32);  // 32-channel blocks in use
  const TilePixel px = tile_pixel(t, r16::kTS, tid);
  const int64_t pix = pixel_index(a, t, tid);

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
            const FwdRecord r = fwd_record(s.xy[k], s.con[k], px.fx, px.fy);
            if (blends(r)) {
              const float next_T = T * (1.f - r.alpha);
              if (next_T <= kTMin) {
                done = true;
              } else {
                w = r.alpha * T;
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

  if (slab == 0 && pix >= 0) {
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
__global__ void __launch_bounds__(256) wide_bwd_kernel(TileArgs a, int nslab) {
  __shared__ Geom<kBatch> s;
  __shared__ float s_vout[256 * kBwdLd];  // v_out[pixel][channel] of the tile and slab
  __shared__ float s_col[kBatch * kBwdLd];
  __shared__ float s_qw[kBatch * kWLd];  // q, then w, [Gaussian][pixel]
  __shared__ float s_qa[ABS ? kBatch * kWLd : 1];  // q over all channels (see `multi`)
  __shared__ int32_t s_maxlast[4];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int i = lane & 15, j = lane >> 4;
  // workgroup = (tile, slab): blockIdx.x = tile * nslab + slab
  const int tile = blockIdx.x / nslab, slab = blockIdx.x - tile * nslab;
  const TileCtx t = tile_ctx(a, tile, r16::kTS, a.n_tiles);
  if (a.masks && a.masks[t.tile]) return;
  const int ch0 = slab * kBwdSlab;
  const int nch = min(kBwdSlab, a.D - ch0);
  const int ksteps = (nch + 3) / 4;
  const TilePixel px = tile_pixel(t, r16::kTS, tid);
  const int64_t pix = pixel_index(a, t, tid);

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
    if (slab == 0 && a.v_render_alphas) Dra = a.v_render_alphas[pix];
    my_last = a.last_ids[pix];
  }
  const int32_t max_last = tile_max_last(my_last, s_maxlast, 4);
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
  const bool multi = ABS && nslab > 1 && slab == 0;
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
      const float2 xy = s.xy[k];  // before cn: the order of the loads is that of the operands
      const float4 cn = s.con[k];
      const BwdRecord r = bwd_record(xy, cn, px.fx, px.fy);
      const bool valid = (idx <= my_last) && blends(r);
      float w = 0.f;
      if (__ballot(valid) != 0) {
        float g[NF];
#pragma unroll
        for (int f = 0; f < NF; ++f) g[f] = 0.f;
        if (valid) {
          const float alpha = fminf(kAlphaMax, r.alpha_raw);
          const float ra = 1.f / (1.f - alpha);
          T *= ra;
          w = alpha * T;
          const float q = s_qw[k * kWLd + tid];
          rD += q * w;
          float Dalpha = ra * (fin + T * q - rD);
          if (r.alpha_raw > kAlphaMax) Dalpha = 0.f;  // a clamped alpha has no gradient
          const GeomGrads gg = geom_grads(cn, r, alpha, Dalpha);
          g[0] = gg.op, g[1] = gg.mx, g[2] = gg.my, g[3] = gg.ca, g[4] = gg.cb, g[5] = gg.cc;
          if constexpr (ABS) {
            if (slab == 0) {
              const float qa = multi ? s_qa[k * kWLd + tid] : q;
              rD_a += qa * w;
              float Da = ra * (fin_a + T * qa - rD_a);
              if (r.alpha_raw > kAlphaMax) Da = 0.f;
              const float aDa = alpha * Da;
              g[6] = fabsf(aDa * (cn.x * r.dx + cn.y * r.dy));
              g[7] = fabsf(aDa * (cn.y * r.dx + cn.z * r.dy));
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
  GS_REQUIRE(n_isects >= 0, "%s: negative sizes", who);
  if (int e = check_tile_sizes(who, C, W, H, ts, tw, th)) return e;
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
  const TileArgs a = tile_args(C, D, width, height, tile_size, tile_width, tile_height, means2d,
                               conics, colors, opacities, backgrounds, masks, isect_offsets,
                               n_isects, flatten_ids, render_colors, render_alphas, last_ids);
  if (a.n_tiles == 0) return 0;
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
  const TileArgs a = tile_args(C, D, width, height, tile_size, tile_width, tile_height, means2d,
                               conics, colors, opacities, backgrounds, masks, isect_offsets,
                               n_isects, flatten_ids, nullptr, const_cast<float *>(render_alphas),
                               const_cast<int32_t *>(last_ids), v_render_colors, v_render_alphas,
                               v_means2d, v_conics, v_colors, v_opacities, v_means2d_abs);
  if (int e = zero_grads(a, n_gaussians, st)) return e;
  if (a.n_tiles == 0 || n_isects == 0) return 0;
  const int nslab = (D + wide::kBwdSlab - 1) / wide::kBwdSlab;
  const dim3 grid((unsigned)(a.n_tiles * nslab));
  if (v_means2d_abs)
    hipLaunchKernelGGL(wide::wide_bwd_kernel<true>, grid, dim3(256), 0, st, a, nslab);
  else
    hipLaunchKernelGGL(wide::wide_bwd_kernel<false>, grid, dim3(256), 0, st, a, nslab);
  GS_CHECK_LAUNCH("rasterize_wide_bwd");
  return 0;
}
