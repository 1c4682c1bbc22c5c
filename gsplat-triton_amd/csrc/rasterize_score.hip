// Per-Gaussian contribution scores of the 16x16 rasterizer (gfx950): the
// forward's walk over a tile's depth-sorted records, reduced over the PIXELS
// per Gaussian instead of over the Gaussians per pixel.  For every record the
// kernel adds, to its Gaussian's row,
//   sum   += sum over the tile's pixels of w (times the pixel's weight),
//   max    = max(max, largest w over the tile's pixels),
//   count += pixels that blended it,
// with w = alpha * T exactly where the forward (rasterize16.hip) blends:
// s2 = sigma * log2(e) from conics pre-scaled at staging, alpha =
// min(0.999, opacity * 2^-s2), blended iff 0 <= s2 <= log2(255 opacity) and
// T (1 - alpha) > 1e-4 (exclusive stop), pixel centres at +0.5.
//
// One workgroup per tile, 256 lanes, lane l of wave w owns pixel (l & 15,
// 4 w + (l >> 4)) as in the forward.  Per batch of 64 records:
//   stage   the four waves gather one attribute group each (mean, conic,
//           opacity, row) of the 64 records into LDS, 8 dwords per record
//           (x, y, A, B | C, opacity, smax, row): two ds_read_b128 with a
//           wave-uniform address per record in the walk;
//   walk    every lane composites the batch in four groups of 16 records and
//           keeps the group's 16 weights in registers;
//   reduce  per group, three reduce-scatters over the wave's 64 pixels
//           (wave_ops.h: permlane32/16 swaps and DPP row rotations, 15
//           combining steps + 2 quad steps for 16 fields): weighted sum, max
//           and count (as a float: <= 64, exact).  A quad of lanes ends with
//           the same 16 totals, so lane l keeps group (l & 3): after the four
//           groups lane l owns record 16 (l & 3) + rs_field(l) of the batch;
//   merge   the waves' 3 x 64 partials meet in LDS; thread (q, j) of the
//           first 192 combines quantity q of record j over the four waves
//           and issues ONE global atomic, and none when no pixel of the tile
//           blended the record.
// A wave whose pixels have all terminated skips walk and reduce (it still
// helps staging, which is shared); the workgroup leaves when all four have.
#include "raster_tile.h"
#include "wave_ops.h"

#include "../../include/gsplat_hip.h"

namespace gs {
namespace score {

constexpr int kTS = 16;
constexpr int kBatch = 64;
constexpr int kGroup = 16;  // records per reduce-scatter
constexpr float kLog2e = 1.4426950408889634f;

struct Args {
  int C, N, W, H, tw, th, n_tiles, fold;
  int64_t n_isects;
  const float *means2d, *conics, *opacities, *pixel_weights;
  const uint8_t *masks;
  const int32_t *offsets, *flatten_ids;
  float *sum, *max;
  int32_t *count;
};

__global__ void __launch_bounds__(256) score_kernel(const Args a) {
  // staged records, double-buffered: batch b + 1 is staged while a slower
  // wave still reads batch b's rows in the merge
  __shared__ float4 s_rec[2][kBatch][2];
  __shared__ float s_red[4][3][kBatch];  // per wave: sum, max, count of the batch's records
  __shared__ int s_alive[4];

  const int tile = blockIdx.x;
  if (a.masks && a.masks[tile]) return;  // a skipped tile, as in the forward
  const int start = a.offsets[tile];
  const int end = tile == a.n_tiles - 1 ? (int)a.n_isects : a.offsets[tile + 1];
  if (start >= end) return;

  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int ntile = a.tw * a.th;
  const int c = tile / ntile;
  const int rem = tile - c * ntile;
  const int ty = rem / a.tw, tx = rem - ty * a.tw;
  const int px = tx * kTS + (lane & 15), py = ty * kTS + 4 * wv + (lane >> 4);
  const bool inside = px < a.W && py < a.H;
  const float fx = (float)px + 0.5f, fy = (float)py + 0.5f;
  float pw = 1.f;
  if (a.pixel_weights && inside) pw = a.pixel_weights[((int64_t)c * a.H + py) * a.W + px];
  // a finished (or outside) pixel carries a negative T, as in the forward
  float T = inside ? 1.f : -1.f;
  // the record this lane owns after the four reduce-scatters of a batch
  const int own = kGroup * (lane & 3) + rs_field(lane);

  int buf = 0;
  for (int b0 = start; b0 < end; b0 += kBatch, buf ^= 1) {
    {  // stage: wave wv gathers attribute group wv of record `lane`
      const int idx = b0 + lane;
      const bool valid = idx < end;
      const int64_t g = valid ? a.flatten_ids[idx] : 0;
      const float op = valid ? a.opacities[g] : 0.f;
      // opacity < 1/255 (or NaN) never reaches alpha >= 1/255: a pad record,
      // as the forward's strip test drops it (x = NaN never hits)
      const bool ok = valid && op >= kAlphaMin;
      float *r = reinterpret_cast<float *>(&s_rec[buf][lane][0]);
      if (wv == 0) {
        const float2 xy = ok ? reinterpret_cast<const float2 *>(a.means2d)[g] : float2{0.f, 0.f};
        r[0] = ok ? xy.x : __int_as_float(0x7fc00000);
        r[1] = xy.y;
      } else if (wv == 1) {
        const float *cn = a.conics + 3 * g;
        r[2] = ok ? 0.5f * kLog2e * cn[0] : 0.f;
        r[3] = ok ? kLog2e * cn[1] : 0.f;
        r[4] = ok ? 0.5f * kLog2e * cn[2] : 0.f;
      } else if (wv == 2) {
        r[5] = ok ? op : 0.f;
        r[6] = ok ? fmaxf(__builtin_amdgcn_logf(255.f * op), 0.f) : 0.f;  // log2; never negative bits
      } else {
        r[7] = __int_as_float(ok ? (int)(a.fold ? g % a.N : g) : -1);
      }
    }
    __syncthreads();

    bool alive = __ballot(T > 0.f) != 0;
    float ms = 0.f, mm = 0.f, mc = 0.f;
    if (alive) {
#pragma unroll
      for (int grp = 0; grp < kBatch / kGroup; ++grp) {
        // wave-uniform: the group holds records and some pixel is alive
        if (b0 + grp * kGroup >= end || __ballot(T > 0.f) == 0) break;
        float w[kGroup], ws[kGroup], wc[kGroup];
#pragma unroll
        for (int i = 0; i < kGroup; ++i) {
          const float4 r0 = s_rec[buf][grp * kGroup + i][0];
          const float4 r1 = s_rec[buf][grp * kGroup + i][1];
          const float dx = r0.x - fx, dy = r0.y - fy;
          const float s2 = __builtin_fmaf(
              dx, __builtin_fmaf(r0.z, dx, r0.w * dy), r1.x * dy * dy);
          const float al = fminf(r1.y * __builtin_amdgcn_exp2f(-s2), kAlphaMax);
          const bool hit = __float_as_uint(s2) <= __float_as_uint(r1.z);  // 0 <= s2 <= smax
          const float nT = __builtin_fmaf(-T, al, T);  // T (1 - alpha); negative for a dead pixel
          const bool gt = nT > kTMin;
          const bool blend = hit & gt;
          w[i] = blend ? al * T : 0.f;
          ws[i] = w[i] * pw;
          wc[i] = blend ? 1.f : 0.f;
          // hit but T would drop to <= 1e-4: exclusive stop
          T = blend ? nT : (hit ? -fabsf(T) : T);
        }
        const float zs = reduce_scatter<kGroup>(ws, lane);
        const float zm = reduce_scatter<kGroup, Max>(w, lane);
        const float zc = reduce_scatter<kGroup>(wc, lane);
        if ((lane & 3) == grp) ms = zs, mm = zm, mc = zc;
      }
      alive = __ballot(T > 0.f) != 0;
    }
    // lanes of a quad own four different records, so `own` is a permutation
    // of 0..63: every slot is written, by zeros where nothing was walked
    s_red[wv][0][own] = ms;
    s_red[wv][1][own] = mm;
    s_red[wv][2][own] = mc;
    if (lane == 0) s_alive[wv] = alive;
    __syncthreads();

    if (wv < 3) {  // thread (wv, lane): quantity wv of record `lane`
      const float cnt = s_red[0][2][lane] + s_red[1][2][lane] + s_red[2][2][lane] +
                        s_red[3][2][lane];
      if (cnt > 0.f) {
        const int64_t row = __float_as_int(reinterpret_cast<const float *>(&s_rec[buf][lane][1])[3]);
        const float v0 = s_red[0][wv][lane], v1 = s_red[1][wv][lane];
        const float v2 = s_red[2][wv][lane], v3 = s_red[3][wv][lane];
        if (wv == 0)
          atomic_add_f32(a.sum + row, (v0 + v1) + (v2 + v3));
        else if (wv == 1)  // w >= 0: the order of the bits is the order of the values
          atomicMax(reinterpret_cast<int *>(a.max) + row,
                    __float_as_int(fmaxf(fmaxf(v0, v1), fmaxf(v2, v3))));
        else
          atomicAdd(a.count + row, (int)cnt);
      }
    }
    if (!(s_alive[0] | s_alive[1] | s_alive[2] | s_alive[3])) break;
  }
}

}  // namespace score
}  // namespace gs

extern "C" int gsplat_hip_rasterize_score(int C, int N, int64_t n_rows, int W, int H,
                                          int tile_size, int tile_width, int tile_height,
                                          const float *means2d, const float *conics,
                                          const float *opacities, const uint8_t *masks,
                                          const float *pixel_weights, const int32_t *offsets,
                                          int64_t n_isects, const int32_t *flatten_ids, int fold,
                                          int accumulate, float *sum, float *max, int32_t *count,
                                          void *stream) {
  using namespace gs;
  const char *name = "rasterize_score";
  GS_REQUIRE(tile_size == score::kTS, "%s: tile_size must be 16, got %d", name, tile_size);
  GS_REQUIRE(C >= 0 && N >= 0 && n_rows >= 0 && W > 0 && H > 0, "%s: bad sizes", name);
  GS_REQUIRE(tile_width * tile_size >= W && tile_height * tile_size >= H,
             "%s: the tile grid does not cover the image", name);
  GS_REQUIRE(n_isects >= 0 && n_isects <= 0x7fffffff, "%s: n_isects beyond int32", name);
  GS_REQUIRE(!fold || N > 0, "%s: fold needs N", name);
  GS_REQUIRE(sum && max && count, "%s: null output", name);
  const int64_t n_tiles = (int64_t)C * tile_width * tile_height;
  GS_REQUIRE(n_tiles <= 0x7fffffff, "%s: too many tiles", name);
  hipStream_t st = (hipStream_t)stream;
  if (!accumulate) {
    GS_HIP(zero_async(sum, (size_t)n_rows * 4, st));
    GS_HIP(zero_async(max, (size_t)n_rows * 4, st));
    GS_HIP(zero_async(count, (size_t)n_rows * 4, st));
  }
  if (n_isects == 0 || n_tiles == 0 || n_rows == 0) return 0;
  GS_REQUIRE(means2d && conics && opacities && offsets && flatten_ids, "%s: null input", name);
  score::Args a;
  a.C = C, a.N = N, a.W = W, a.H = H, a.tw = tile_width, a.th = tile_height;
  a.n_tiles = (int)n_tiles, a.fold = fold, a.n_isects = n_isects;
  a.means2d = means2d, a.conics = conics, a.opacities = opacities;
  a.pixel_weights = pixel_weights, a.masks = masks, a.offsets = offsets;
  a.flatten_ids = flatten_ids, a.sum = sum, a.max = max, a.count = count;
  hipLaunchKernelGGL(score::score_kernel, dim3((unsigned)n_tiles), dim3(256), 0, st, a);
  GS_CHECK_LAUNCH(name);
  return 0;
}
