// Tile rasterizer: front-to-back alpha compositing (forward) and its reverse
// sweep (backward) for gfx950.
//
// Replaces the reference Triton kernels
//   rasterize_to_pixels_fwd_kernel  gsplat/triton_impl/rasterize_to_pixels_fwd.py:13-196
//   rasterize_to_pixels_bwd_kernel  gsplat/triton_impl/rasterize_to_pixels_bwd.py:13-337
//
// Mapping (CDNA4): one workgroup per image tile, one lane per pixel (16x16
// tile = 4 wave64s).  The tile's depth-sorted Gaussian list is streamed
// through LDS in batches of up to 256 records staged with one coalesced
// gather per lane (id -> xy, conic+opacity, D colours); every lane then reads
// each record with a broadcast ds_read.  The forward keeps transmittance
// multiplicatively (T *= 1 - alpha) with the reference's exclusive stop at
// T <= 1e-4; `last_ids` is the global isect index of the last contributor.
// The backward walks the same records back to front, rebuilding T from
// T_final, and reduces every per-Gaussian gradient across the wave with a
// butterfly before one fp32 atomic per wave and field.
//
// The argument block, the tile and pixel walk, the geometry staging and the
// per-record alpha steps are raster_tile.h's, shared with rasterize_wide.hip.
#include "raster16.h"
#include "../../include/gsplat_hip.h"

namespace gs {

constexpr int kMaxBatch = 256;

template <int D>
struct Stage : Geom<kMaxBatch> {
  float col[kMaxBatch][D];
};

template <int D>
GS_INLINE void stage_batch(const TileArgs &a, Stage<D> &s, int64_t b0, int nb) {
  stage_geom(a, s, b0, nb);
  const int j = threadIdx.x;
  if (j < nb) {
    // the id from flatten_ids again (one load with stage_geom's), not back from LDS
    const float *cl = a.colors + (int64_t)a.flatten_ids[b0 + j] * D;
#pragma unroll
    for (int d = 0; d < D; ++d) s.col[j][d] = cl[d];
  }
}

template <int D>
__global__ void __launch_bounds__(256) rasterize_fwd_kernel(TileArgs a) {
  __shared__ Stage<D> s;
  const TileCtx t = tile_ctx(a, blockIdx.x, a.ts, a.C * a.tw * a.th);
  // lanes past ts * ts have no pixel: 12- and 4-pixel tiles do not fill their waves
  const TilePixel px = tile_pixel(t, a.ts, threadIdx.x);
  const bool inside = (int)threadIdx.x < a.ts * a.ts && in_image(a, px);
  const int batch = min((int)blockDim.x, kMaxBatch);

  float T = 1.f;
  float acc[D];
#pragma unroll
  for (int d = 0; d < D; ++d) acc[d] = 0.f;
  int32_t last = 0;

  // Tile masks follow the Triton backend: masks[tile] == true skips the tile
  // (rasterize_to_pixels_fwd.py:54-58); its pixels are written as background.
  const bool skip_tile = a.masks && a.masks[t.tile];
  bool done = !inside || skip_tile;

  if (!skip_tile) {
    for (int64_t b0 = t.start; b0 < t.end; b0 += batch) {
      // every pixel terminated -> the whole tile stops (also the LDS WAR fence)
      if (__syncthreads_count(!done) == 0) break;
      const int nb = (int)min((int64_t)batch, t.end - b0);
      stage_batch<D>(a, s, b0, nb);
      __syncthreads();
      if (!done) {
        for (int k = 0; k < nb; ++k) {
          const FwdRecord r = fwd_record(s.xy[k], s.con[k], px.fx, px.fy);
          if (!blends(r)) continue;
          const float next_T = T * (1.f - r.alpha);
          if (next_T <= kTMin) {
            done = true;
            break;
          }
          const float vis = r.alpha * T;
#pragma unroll
          for (int d = 0; d < D; ++d) acc[d] += vis * s.col[k][d];
          T = next_T;
          last = (int32_t)(b0 + k);
        }
      }
    }
  }

  if (inside) {
    const int64_t pix = image_index(a, t, px);
    float *oc = a.render_colors + pix * D;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const float bg = a.backgrounds ? a.backgrounds[t.c * D + d] : 0.f;
      oc[d] = acc[d] + T * bg;
    }
    a.render_alphas[pix] = 1.f - T;
    a.last_ids[pix] = last;
  }
}

template <int D, bool ABS>
__global__ void __launch_bounds__(256) rasterize_bwd_kernel(TileArgs a) {
  __shared__ Stage<D> s;
  __shared__ int32_t s_maxlast[4];
  const TileCtx t = tile_ctx(a, blockIdx.x, a.ts, a.C * a.tw * a.th);
  // lanes past ts * ts have no pixel: 12- and 4-pixel tiles do not fill their waves
  const TilePixel px = tile_pixel(t, a.ts, threadIdx.x);
  const bool inside = (int)threadIdx.x < a.ts * a.ts && in_image(a, px);
  if (a.masks && a.masks[t.tile]) return;
  const int batch = min((int)blockDim.x, kMaxBatch);
  const int lane = threadIdx.x & 63;
  const int64_t pix = image_index(a, t, px);

  float T_final = 1.f, Dra = 0.f, Drc[D];
  int32_t my_last = -1;
#pragma unroll
  for (int d = 0; d < D; ++d) Drc[d] = 0.f;
  if (inside) {
    T_final = 1.f - a.render_alphas[pix];
    Dra = a.v_render_alphas ? a.v_render_alphas[pix] : 0.f;  // null: alphas unused
    my_last = a.last_ids[pix];
#pragma unroll
    for (int d = 0; d < D; ++d) Drc[d] = a.v_render_colors[pix * D + d];
  }
  float bg_term = 0.f;
  if (a.backgrounds) {
#pragma unroll
    for (int d = 0; d < D; ++d) bg_term += a.backgrounds[t.c * D + d] * Drc[d];
    bg_term *= T_final;
  }

  const int32_t max_last = tile_max_last(my_last, s_maxlast, (int)(blockDim.x >> 6));
  const int64_t end = min(t.end, (int64_t)max_last + 1);

  float T = T_final;  // exclusive transmittance of the Gaussian being visited
  float rD = 0.f;     // sum over visited Gaussians of (colour . Drc) * T * alpha

  for (int64_t b1 = end; b1 > t.start; b1 -= batch) {
    const int64_t b0 = max(t.start, b1 - batch);
    const int nb = (int)(b1 - b0);
    __syncthreads();  // previous batch fully consumed
    stage_batch<D>(a, s, b0, nb);
    __syncthreads();
    for (int k = nb - 1; k >= 0; --k) {
      const int64_t idx = b0 + k;
      const float4 cn = s.con[k];
      const BwdRecord r = bwd_record(s.xy[k], cn, px.fx, px.fy);
      const bool valid = inside && (idx <= my_last) && blends(r);
      if (__ballot(valid) == 0) continue;  // wave-uniform skip

      float g_col[D], g_ax = 0.f, g_ay = 0.f;
      GeomGrads g = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int d = 0; d < D; ++d) g_col[d] = 0.f;
      if (valid) {
        const float alpha = fminf(kAlphaMax, r.alpha_raw);
        const float ra = 1.f / (1.f - alpha);
        T *= ra;
        const float w = alpha * T;
        float gD = 0.f;
#pragma unroll
        for (int d = 0; d < D; ++d) {
          g_col[d] = w * Drc[d];
          gD += s.col[k][d] * Drc[d];
        }
        rD += gD * w;
        float Dalpha = ra * (T_final * Dra + T * gD - rD - bg_term);
        if (r.alpha_raw > kAlphaMax) Dalpha = 0.f;  // clamped alpha has no gradient
        g = geom_grads(cn, r, alpha, Dalpha);
        if (ABS) {
          g_ax = fabsf(g.mx);
          g_ay = fabsf(g.my);
        }
      }
#pragma unroll
      for (int d = 0; d < D; ++d) g_col[d] = wave_sum(g_col[d]);
      g.op = wave_sum(g.op);
      g.mx = wave_sum(g.mx);
      g.my = wave_sum(g.my);
      g.ca = wave_sum(g.ca);
      g.cb = wave_sum(g.cb);
      g.cc = wave_sum(g.cc);
      if (ABS) {
        g_ax = wave_sum(g_ax);
        g_ay = wave_sum(g_ay);
      }
      if (lane == 0) {
        const int64_t gi = s.gid[k];
#pragma unroll
        for (int d = 0; d < D; ++d) atomic_add_f32(a.v_colors + gi * D + d, g_col[d]);
        atomic_add_f32(a.v_opacities + gi, g.op);
        atomic_add_f32(a.v_means2d + 2 * gi, g.mx);
        atomic_add_f32(a.v_means2d + 2 * gi + 1, g.my);
        atomic_add_f32(a.v_conics + 3 * gi, g.ca);
        atomic_add_f32(a.v_conics + 3 * gi + 1, g.cb);
        atomic_add_f32(a.v_conics + 3 * gi + 2, g.cc);
        if (ABS) {
          atomic_add_f32(a.v_abs + 2 * gi, g_ax);
          atomic_add_f32(a.v_abs + 2 * gi + 1, g_ay);
        }
      }
    }
  }
}

template <int D>
int launch_fwd(const TileArgs &a, int threads, hipStream_t st) {
  hipLaunchKernelGGL(rasterize_fwd_kernel<D>, dim3(a.C * a.tw * a.th), dim3(threads), 0, st, a);
  GS_CHECK_LAUNCH("rasterize_fwd");
  return 0;
}

template <int D>
int launch_bwd(const TileArgs &a, int threads, hipStream_t st) {
  if (a.v_abs)
    hipLaunchKernelGGL((rasterize_bwd_kernel<D, true>), dim3(a.C * a.tw * a.th), dim3(threads), 0,
                       st, a);
  else
    hipLaunchKernelGGL((rasterize_bwd_kernel<D, false>), dim3(a.C * a.tw * a.th), dim3(threads),
                       0, st, a);
  GS_CHECK_LAUNCH("rasterize_bwd");
  return 0;
}

inline bool supported_channels(int D) {
#define GS_CASE(n) if (D == n) return true;
  GS_RASTER_CHANNELS(GS_CASE)
#undef GS_CASE
  return false;
}

}  // namespace gs

using namespace gs;

extern "C" int gsplat_hip_rasterize_supported_channels(int D) { return supported_channels(D); }

// 16x16 tiles (the gsplat default) run the wave-per-tile kernels of
// rasterize16.hip (its entries: raster16.h); other tile sizes run the
// workgroup-per-tile kernels here.
extern "C" int64_t gsplat_hip_rasterize_fwd_state_bytes(int C, int D, int tile_size,
                                                        int tile_width, int tile_height,
                                                        int64_t n_isects) {
  if (tile_size != 16 || !supported_channels(D)) return 0;
  return rasterize16_fwd_state_bytes(D, C * tile_width * tile_height, n_isects);
}

extern "C" int gsplat_hip_rasterize_prepare(int C, int D, int tile_size, int tile_width,
                                           int tile_height, const int32_t *isect_offsets,
                                           int64_t n_isects, const int64_t *n_isects_device,
                                           void *state, int64_t state_bytes, void *stream) {
  if (tile_size != 16 || !supported_channels(D)) return 0;
  return rasterize16_prepare(D, C, tile_width, tile_height, isect_offsets, n_isects,
                             n_isects_device, state, state_bytes, (hipStream_t)stream);
}

extern "C" int64_t gsplat_hip_rasterize_bwd_workspace_bytes(int64_t n_gaussians, int D,
                                                            int tile_size, int absgrad, int C,
                                                            int tile_width, int tile_height,
                                                            int64_t n_isects) {
  if (tile_size != 16 || !supported_channels(D)) return 0;
  return rasterize16_bwd_workspace(n_gaussians, D, absgrad != 0, C * tile_width * tile_height,
                                   n_isects);
}

extern "C" int gsplat_hip_rasterize_record_floats(int D, int tile_size) {
  return tile_size == 16 ? rasterize16_record_floats(D) : 0;
}

extern "C" int gsplat_hip_rasterize_pack_records(int64_t n_gaussians, int D, const float *means2d,
                                                 const float *conics, const float *colors,
                                                 const float *opacities, const int32_t *visible,
                                                 const int32_t *vis_rank, float *records,
                                                 void *stream) {
  GS_REQUIRE(!vis_rank || visible, "rasterize_pack_records: vis_rank needs visible");
  return rasterize16_pack_records(n_gaussians, D, means2d, conics, colors, opacities, visible,
                                  vis_rank, records, (hipStream_t)stream);
}

static int check_common(int C, int D, int W, int H, int ts, int tw, int th) {
  GS_REQUIRE(supported_channels(D), "rasterize: unsupported channel count %d", D);
  GS_REQUIRE(ts > 0 && ts * ts <= 256, "rasterize: tile_size %d not in [1, 16]", ts);
  return check_tile_sizes("rasterize", C, W, H, ts, tw, th);
}

static int block_threads(int ts) { return ((ts * ts + 63) / 64) * 64; }

extern "C" int gsplat_hip_rasterize_fwd(int C, int D, int width, int height, int tile_size,
                                        int tile_width, int tile_height, const float *means2d,
                                        const float *conics, const float *colors,
                                        const float *opacities, const float *backgrounds,
                                        const uint8_t *masks, const int32_t *isect_offsets,
                                        int64_t n_isects, const int64_t *n_isects_device,
                                        const int32_t *flatten_ids, float *render_colors,
                                        float *render_alphas, int32_t *last_ids,
                                        const float *records, void *state, int64_t state_bytes,
                                        void *stream) {
  if (int e = check_common(C, D, width, height, tile_size, tile_width, tile_height)) return e;
  GS_REQUIRE(tile_size == 16 || !n_isects_device,
             "rasterize_fwd: a device isect count needs 16x16 tiles");
  if ((int64_t)C * tile_width * tile_height == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (tile_size == 16)
    return rasterize16_fwd(C, D, width, height, tile_width, tile_height, means2d, conics, colors,
                           opacities, backgrounds, masks, isect_offsets, n_isects,
                           n_isects_device, flatten_ids, render_colors, render_alphas, last_ids,
                           records, state, state_bytes, st);
  const TileArgs a = tile_args(C, D, width, height, tile_size, tile_width, tile_height, means2d,
                               conics, colors, opacities, backgrounds, masks, isect_offsets,
                               n_isects, flatten_ids, render_colors, render_alphas, last_ids);
  const int thr = block_threads(tile_size);
#define GS_CASE(n) if (D == n) return launch_fwd<n>(a, thr, st);
  GS_RASTER_CHANNELS(GS_CASE)
#undef GS_CASE
  return 1;
}

// Gradient buffers are zeroed here (on `stream`) before accumulation.
extern "C" int gsplat_hip_rasterize_bwd(
    int C, int64_t n_gaussians, int D, int width, int height, int tile_size, int tile_width,
    int tile_height, const float *means2d, const float *conics, const float *colors,
    const float *opacities, const float *backgrounds, const uint8_t *masks,
    const int32_t *isect_offsets, int64_t n_isects, const int64_t *n_isects_device,
    const int32_t *flatten_ids, const float *render_alphas, const int32_t *last_ids,
    const float *v_render_colors,
    const float *v_render_alphas, float *v_means2d, float *v_conics, float *v_colors,
    float *v_opacities, float *v_means2d_abs, const float *render_colors, const float *records,
    const void *state, int64_t state_bytes, void *workspace, int64_t workspace_bytes,
    const int32_t *visible, const int32_t *vis_rank, void *stream) {
  if (int e = check_common(C, D, width, height, tile_size, tile_width, tile_height)) return e;
  GS_REQUIRE(tile_size == 16 || !n_isects_device,
             "rasterize_bwd: a device isect count needs 16x16 tiles");
  hipStream_t st = (hipStream_t)stream;
  if (tile_size == 16) {
    const int64_t need = rasterize16_bwd_workspace(n_gaussians, D, v_means2d_abs != nullptr,
                                                   C * tile_width * tile_height, n_isects);
    GS_REQUIRE(workspace_bytes >= need && (need == 0 || workspace),
               "rasterize_bwd: workspace of %lld bytes needed, %lld given", (long long)need,
               (long long)workspace_bytes);
    return rasterize16_bwd(C, n_gaussians, D, width, height, tile_width, tile_height, means2d,
                           conics, colors, opacities, backgrounds, masks, isect_offsets,
                           n_isects, n_isects_device, flatten_ids, render_alphas, last_ids,
                           v_render_colors,
                           v_render_alphas, v_means2d, v_conics, v_colors, v_opacities,
                           v_means2d_abs, render_colors, records, state, state_bytes, workspace,
                           visible, vis_rank, st);
  }
  const TileArgs a = tile_args(C, D, width, height, tile_size, tile_width, tile_height, means2d,
                               conics, colors, opacities, backgrounds, masks, isect_offsets,
                               n_isects, flatten_ids, nullptr, const_cast<float *>(render_alphas),
                               const_cast<int32_t *>(last_ids), v_render_colors, v_render_alphas,
                               v_means2d, v_conics, v_colors, v_opacities, v_means2d_abs);
  if (int e = zero_grads(a, n_gaussians, st)) return e;
  if ((int64_t)C * tile_width * tile_height == 0 || n_isects == 0) return 0;
  const int thr = block_threads(tile_size);
#define GS_CASE(n) if (D == n) return launch_bwd<n>(a, thr, st);
  GS_RASTER_CHANNELS(GS_CASE)
#undef GS_CASE
  return 1;
}
