// What the 16x16 rasterizer's files agree on: the kernels' argument block and
// constants, the entries the C ABI (rasterize.hip) calls, and what the kernel
// side (rasterize16.hip) asks of the planning side (rasterize16_plan.hip).
#pragma once

#include "common.h"

// Colour channel counts with compiled forward and backward kernels, for every
// tile size (the caller pads others).
#define GS_RASTER_CHANNELS(X) X(1) X(2) X(3) X(4) X(8) X(16) X(32)

namespace gs {

// ---- entries, called by rasterize.hip for tile_size == 16
int rasterize16_fwd(int C, int D, int W, int H, int tw, int th, const float *means2d,
                    const float *conics, const float *colors, const float *opacities,
                    const float *backgrounds, const uint8_t *masks, const int32_t *offsets,
                    int64_t n_isects, const int64_t *n_isects_dev, const int32_t *flatten_ids,
                    float *render_colors, float *render_alphas, int32_t *last_ids,
                    const float *records, void *state, int64_t state_bytes, hipStream_t st);
int rasterize16_bwd(int C, int64_t G, int D, int W, int H, int tw, int th,
                    const float *means2d, const float *conics, const float *colors,
                    const float *opacities, const float *backgrounds, const uint8_t *masks,
                    const int32_t *offsets, int64_t n_isects, const int64_t *n_isects_dev,
                    const int32_t *flatten_ids, const float *render_alphas,
                    const int32_t *last_ids, const float *v_render_colors,
                    const float *v_render_alphas, float *v_means2d, float *v_conics,
                    float *v_colors, float *v_opacities, float *v_abs, const float *render_colors,
                    const float *records, const void *state, int64_t state_bytes,
                    void *workspace, const int32_t *visible, const int32_t *vis_rank,
                    hipStream_t st);
int rasterize16_record_floats(int D);
int rasterize16_pack_records(int64_t G, int D, const float *means2d, const float *conics,
                             const float *colors, const float *opacities, const int32_t *visible,
                             const int32_t *vis_rank, float *records, hipStream_t st);
// (rasterize16_plan.hip)
int64_t rasterize16_fwd_state_bytes(int D, int n_tiles, int64_t n_isects);
int rasterize16_prepare(int D, int C, int tw, int th, const int32_t *offsets, int64_t n_isects,
                        const int64_t *n_isects_dev, void *state, int64_t state_bytes,
                        hipStream_t st);
int64_t rasterize16_bwd_workspace(int64_t G, int D, bool absgrad, int n_tiles, int64_t n_isects);

namespace r16 {

constexpr int kTS = 16;
constexpr float kAlphaMin = 1.f / 255.f;
constexpr float kAlphaMax = 0.999f;
constexpr float kTMin = 1e-4f;

// Render records: one 64-B row per Gaussian, [x, y, a, b, c, opacity,
// colour[D], pad] (D <= kRecMaxD), so the per-isect gather of a batch touches
// one 64-B sector per lane instead of four lines of four arrays
// (rasterize_to_pixels_fwd.py:93-145 loads the four arrays separately).
constexpr int kItemRun = 4;  // work items per XCD run (fwd_kernel<SPLIT>, bwd2_kernel)
constexpr int kRecFloats = 16;
constexpr int kRecMaxD = kRecFloats - 6;

struct Args {
  int C, W, H, tw, th, n_tiles;
  int64_t n_isects;  // isect count, or with n_dev the capacity of the isect arrays
  const int64_t *n_dev;  // the isect count on the device (capacity mode) or null
  const float *means2d, *conics, *colors, *opacities, *backgrounds;
  const float *records;  // [G][kRecFloats] render records, or null (gather the arrays)
  uint32_t rec_bytes;    // bytes of the record table (< 2^31: buffer-load offsets)
  const uint8_t *masks;
  const int32_t *offsets, *flatten_ids;
  float *render_colors, *render_alphas;
  int32_t *last_ids;
  const float *v_render_colors, *v_render_alphas;
  float *packed;  // [G][S] gradient rows (backward)
  int S;
  // Chunk states (see "Chunked backward"): slot s = boundary isect index / L
  // holds T[256] then acc[D][256] of the tile's pixels before that isect.
  float *state;
  int L;  // chunk length in isects (multiple of 64); 0 = no chunking
  // backward work items (tile, chunk): n_items[0] full-length chunks at
  // items[0..), n_items[1] tails at items_tail[0..)
  const int2 *items, *items_tail;
  const int32_t *n_items;
  const int32_t *order;  // forward: tile of workgroup b (heaviest tiles first) or null
  const int32_t *n_whole;  // forward: the number of tiles in `order` (device), or null: all
  // forward, split heavy tiles (fwd_plan_kernel, "Split heavy tiles"):
  // fitems[b] = (tile, k), chunk k of a split tile, n_chunks of them (device).
  // prod: per boundary slot (b / L) the product of (1 - alpha) over the chunk
  // ending at b, pflag[4 * slot + wave] its ready flags; cout: per chunk (its
  // index in fitems), the chunk's end T, last id and colour sum [2 + D][256];
  // ctr[index of chunk 0] the tile's finished chunks (chunk START slots are
  // not unique: a tile's first chunk can share b / L with the previous
  // tile's last one).
  const int2 *fitems;
  const int32_t *n_chunks;
  float *prod, *cout;
  int32_t *pflag, *ctr;
  int SL;  // split tiles: isects per chunk (a multiple of L)
  const float *render_colors_in;  // backward: forward colours (for suffix sums)
  int dbg;  // debug flags (gsplat_hip_debug_set_flags): bit 0 = backward skips its
            // atomics, bit 1 = split chunks never wait for a published product
  uint64_t *timeline;  // debug: per-wave (start, end) s_memrealtime stamps or null
};

// Isect count and the end of tile t's isect range.  Capacity mode (n_dev
// non-null, the sync-free isect of a captured training step): the arrays
// hold n_isects slots, the count is read on the device.
GS_INLINE int64_t isect_count(const int64_t *n_dev, int64_t n) { return n_dev ? *n_dev : n; }
GS_INLINE int64_t tile_end(const int32_t *offsets, int t, int n_tiles, const int64_t *n_dev,
                           int64_t n) {
  return t == n_tiles - 1 ? isect_count(n_dev, n) : (int64_t)offsets[t + 1];
}
GS_INLINE int64_t tile_end(const Args &a, int t) {
  return tile_end(a.offsets, t, a.n_tiles, a.n_dev, a.n_isects);
}

// The XCD-grouped order's groups of kGS x kGS neighbouring tiles
// (tile_order_grouped_kernel).
constexpr int kGS = 2;
__host__ __device__ inline int order_groups(int C, int tw, int th) {
  return C * ((tw + kGS - 1) / kGS) * ((th + kGS - 1) / kGS);
}

}  // namespace r16

// ---- rasterize16_plan.hip, for the launches of rasterize16.hip

// Chunk length in isects of the chunked backward (multiple of 64; 0: off).
int chunk_len();
// Bytes of the chunk slots, the head of the forward's state.
int64_t chunk_slot_bytes(int D, int64_t n_isects);
// Bytes of the packed [G][S] gradient rows (256-B aligned) at the head of the
// backward's workspace, and the bound on its work items after them.
size_t packed_bytes(int D, bool absgrad, int64_t G);
int64_t n_items_bound(int n_tiles, int64_t n_isects);

// Points a.L, a.state, a.order and, for a split forward, the split area's
// fields into `state` (null: none of them), and queues the kernel that
// writes the order or the split plan unless rasterize16_prepare already did
// for this state.  split: launch fwd_kernel<D, true>; grid: its workgroups.
struct FwdLaunch {
  bool split;
  unsigned grid;
};
int plan_forward(r16::Args &a, int D, void *state, int64_t state_bytes, hipStream_t st,
                 FwdLaunch &launch);

// Points a.n_items, a.items and a.items_tail of the chunked backward into the
// workspace at items_base (after the gradient rows) and queues the kernel
// that writes them; returns the backward's grid.
int64_t plan_backward(r16::Args &a, char *items_base, hipStream_t st);

}  // namespace gs
