// Planning side of the 16x16 rasterizer (rasterize16.hip has the kernels that
// render): the knobs, the layout of the forward's state and the backward's
// workspace, and the small kernels that decide what each workgroup of the
// forward and the backward works on -- the forward's dispatch order (per
// tile, or per 2x2 group for the XCDs), its plan with split heavy tiles, and
// the backward's work items.
#include "raster16.h"
#include "../../include/gsplat_hip.h"

#include <stdlib.h>

#include <algorithm>

namespace gs {
namespace r16 {

GS_INLINE int64_t tile_count(const int32_t *offsets, int t, int n_tiles, const int64_t *n_dev,
                             int64_t n_isects) {
  return tile_end(offsets, t, n_tiles, n_dev, n_isects) - offsets[t];
}

// The largest tile's isect count -> *out (lane 0 of the block; out may be
// null): read back by the host on a LATER render to decide whether to launch
// the split-capable forward (use_split_now), never for correctness.  Uses
// one barrier.
GS_INLINE void block_max_out(int64_t v, int32_t *out) {
  __shared__ int smax;
  if (threadIdx.x == 0) smax = 0;
  __syncthreads();
  int x = (int)min(v, (int64_t)INT32_MAX);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x = max(x, __shfl_xor(x, o, 64));
  if ((threadIdx.x & 63) == 0) atomicMax(&smax, x);
  __syncthreads();
  if (threadIdx.x == 0 && out) *out = smax;
}

// ---- The forward's dispatch order.  Tiles (or groups of tiles) are bucketed
// by isect count, heaviest bucket first, so the longest tiles start in the
// first wave of workgroups instead of finishing last.  Inside a bucket: lane
// order (lane l of the one 1024-lane workgroup holds items l, l + 1024, ...).
GS_INLINE int bucket_of(int64_t n) { return n >= 2048 ? 0 : n >= 1024 ? 1 : n >= 512 ? 2 : 3; }

// One item of bucket bk among a lane's four counts, 16 bits each in a u64
// (at most 16384 items in all), so that one scan serves the four buckets.
GS_INLINE uint64_t bucket_one(int bk) { return (uint64_t)1 << (16 * bk); }

// Exclusive scan over the workgroup's 1024 lanes: a wave scan, then the 16
// waves' sums through `wsum`.  v: the lane's value on entry, the sum over the
// lanes before it on return; returns the total.  One barrier.
template <class T>
GS_INLINE T block_scan(T &v, T (&wsum)[16]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  T x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) wsum[w] = x;
  __syncthreads();
  T before = 0, total = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    before += i < w ? wsum[i] : 0;
    total += wsum[i];
  }
  v = before + (x - v);
  return total;
}

// From a lane's packed bucket counts: pos[bk], the place of its first item of
// bucket bk in the order (the buckets one after the other, heaviest first);
// returns the number of items.
GS_INLINE int bucket_starts(uint64_t mine, uint64_t (&wsum)[16], int (&pos)[4]) {
  const uint64_t total = block_scan(mine, wsum);
  int base = 0;
#pragma unroll
  for (int bk = 0; bk < 4; ++bk) {
    pos[bk] = base + (int)((mine >> (16 * bk)) & 0xffff);
    base += (int)((total >> (16 * bk)) & 0xffff);
  }
  return base;
}

// The place of the lane's next item of bucket bk, and advance (selects: pos
// stays in registers).
GS_INLINE int take(int (&pos)[4], int bk) {
  int p = pos[0];
#pragma unroll
  for (int q = 1; q < 4; ++q) p = bk == q ? pos[q] : p;
#pragma unroll
  for (int q = 0; q < 4; ++q) pos[q] += bk == q;
  return p;
}

// Per-tile order (GSPLAT_HIP_DBG bit 4, and the grids the grouped order does
// not cover).
__global__ void __launch_bounds__(1024)
tile_order_kernel(int n_tiles, const int32_t *__restrict__ offsets, int64_t n_isects,
                  const int64_t *__restrict__ n_dev, int32_t *__restrict__ order,
                  int32_t *__restrict__ max_out) {
  constexpr int MAXPER = 16;  // tiles per thread (n_tiles <= 16384)
  __shared__ uint64_t wsum[16];
  const int tid = threadIdx.x;
  int bucket[MAXPER];
  uint64_t mine = 0;
  int64_t nmax = 0;
#pragma unroll
  for (int i = 0; i < MAXPER; ++i) {
    const int t = tid + 1024 * i;
    bucket[i] = -1;
    if (t < n_tiles) {
      const int64_t n = tile_count(offsets, t, n_tiles, n_dev, n_isects);
      nmax = max(nmax, n);
      bucket[i] = bucket_of(n);
      mine += bucket_one(bucket[i]);
    }
  }
  block_max_out(nmax, max_out);
  int pos[4];
  bucket_starts(mine, wsum, pos);
#pragma unroll
  for (int i = 0; i < MAXPER; ++i)
    if (bucket[i] >= 0) order[take(pos, bucket[i])] = tid + 1024 * i;
}

// XCD-grouped dispatch order: the same heaviest-first buckets, per 2x2 group
// of neighbouring tiles instead of per tile (a group's bucket is its heaviest
// tile's), and the four tiles of group q (q-th in that order) in slots
// 32 (q / 8) + q % 8 + 8 k, k < 4.  Workgroup b runs on XCD b % 8, so a
// group's tiles run on ONE XCD, dispatched together: the Gaussians they share
// (at M3 a visible Gaussian covers ~5.5 tiles) are fetched into one L2 instead
// of up to four.  Slots of missing tiles (image edges) hold -1 (the workgroup
// exits); the grid covers order_slots() = 32 ceil(groups / 8) slots.  Up to 8
// groups per lane (8192 groups).
__global__ void __launch_bounds__(1024)
tile_order_grouped_kernel(int C, int tw, int th, const int32_t *__restrict__ offsets,
                          int64_t n_isects, const int64_t *__restrict__ n_dev,
                          int32_t *__restrict__ order, int32_t *__restrict__ max_out) {
  constexpr int MAXPER = 8;
  __shared__ uint64_t wsum[16];
  const int tid = threadIdx.x;
  const int gw = (tw + kGS - 1) / kGS, gh = (th + kGS - 1) / kGS, ng = C * gw * gh;
  const int n_tiles = C * tw * th;
  // the tiles of group g (-1: outside the grid)
  auto tiles_of = [&](int g, int (&t)[kGS * kGS]) {
    const int c = g / (gw * gh), r = g - c * (gw * gh);
    const int gy = r / gw, gx = r - gy * gw;
#pragma unroll
    for (int k = 0; k < kGS * kGS; ++k) {
      const int ty = gy * kGS + k / kGS, tx = gx * kGS + k % kGS;
      t[k] = (tx < tw && ty < th) ? (c * th + ty) * tw + tx : -1;
    }
  };
  int bucket[MAXPER];
  uint64_t mine = 0;
  int64_t nmax = 0;
#pragma unroll
  for (int i = 0; i < MAXPER; ++i) {
    const int g = tid + 1024 * i;
    bucket[i] = -1;
    if (g < ng) {
      int t[kGS * kGS];
      tiles_of(g, t);
      int64_t gm = 0;
#pragma unroll
      for (int k = 0; k < kGS * kGS; ++k)
        if (t[k] >= 0) gm = max(gm, tile_count(offsets, t[k], n_tiles, n_dev, n_isects));
      nmax = max(nmax, gm);
      bucket[i] = bucket_of(gm);
      mine += bucket_one(bucket[i]);
    }
  }
  block_max_out(nmax, max_out);
  int pos[4];
  bucket_starts(mine, wsum, pos);
  auto slot = [](int q, int k) { return 32 * (q >> 3) + (q & 7) + 8 * k; };
#pragma unroll
  for (int i = 0; i < MAXPER; ++i) {
    if (bucket[i] >= 0) {
      const int q = take(pos, bucket[i]);
      int t[kGS * kGS];
      tiles_of(tid + 1024 * i, t);
#pragma unroll
      for (int k = 0; k < kGS * kGS; ++k) order[slot(q, k)] = t[k];
    }
  }
  // the slots of the group positions past the last group (up to a multiple of 8)
  const int q_end = (ng + 7) & ~7;
  for (int q = ng + tid; q < q_end; q += 1024)
#pragma unroll
    for (int k = 0; k < kGS * kGS; ++k) order[slot(q, k)] = -1;
}

// Forward plan with split heavy tiles, decided on this render's tiles.  A
// tile with more than `split` isects is rendered as ceil(n / SL) chunks that
// run in the same launch as the other tiles (rasterize16.hip, "Split heavy
// tiles"), so the longest tiles no longer serialise the end of the forward.
// Outputs: `order` = the other tiles in tile_order_kernel's order, hdr[0]
// their number; `chunks` = (tile, k) of the split tiles in lane order, a
// tile's chunks consecutive in k, hdr[1] their number; the split tiles'
// hand-off flags and chunk counters cleared.  16 tiles per lane (n_tiles <=
// 16384); a tile is classified again in the write pass, which keeps the 16
// tiles' state out of registers.
__global__ void __launch_bounds__(1024)
fwd_plan_kernel(int n_tiles, const int32_t *__restrict__ offsets, int64_t n_isects,
                const int64_t *__restrict__ n_dev, int SL, int L, int split,
                int32_t *__restrict__ hdr, int32_t *__restrict__ order, int2 *__restrict__ chunks,
                int32_t *__restrict__ pflag, int32_t *__restrict__ ctr,
                int32_t *__restrict__ max_out) {
  constexpr int PER = 16;
  __shared__ uint64_t wsum[16];
  __shared__ int csum[16];
  const int tid = threadIdx.x;
  auto chunks_of = [&](int64_t n) -> int { return n > split ? (int)((n + SL - 1) / SL) : 0; };
  uint64_t mine = 0;  // whole tiles per bucket
  int cpos = 0;       // chunks
  int64_t nmax = 0;
  for (int i = 0; i < PER; ++i) {
    const int t = tid + 1024 * i;
    if (t >= n_tiles) break;
    const int64_t n = tile_count(offsets, t, n_tiles, n_dev, n_isects);
    const int nch = chunks_of(n);
    if (nch == 0) mine += bucket_one(bucket_of(n));
    cpos += nch;
    nmax = max(nmax, n);
  }
  block_max_out(nmax, max_out);
  int pos[4];
  const int n_whole = bucket_starts(mine, wsum, pos);
  const int n_chunks = block_scan(cpos, csum);
  for (int i = 0; i < PER; ++i) {
    const int t = tid + 1024 * i;
    if (t >= n_tiles) break;
    const int64_t n = tile_count(offsets, t, n_tiles, n_dev, n_isects);
    const int nch = chunks_of(n);
    if (nch == 0) {
      order[take(pos, bucket_of(n))] = t;
      continue;
    }
    ctr[cpos] = 0;  // index of chunk 0
    for (int k = 0; k < nch; ++k) {
      chunks[cpos++] = make_int2(t, k);
      if (k < nch - 1) {
        const int64_t sl = ((int64_t)offsets[t] + (int64_t)(k + 1) * SL) / L;
        reinterpret_cast<int4 *>(pflag)[sl] = make_int4(0, 0, 0, 0);
      }
    }
  }
  if (tid == 0) {
    hdr[0] = n_whole;
    hdr[1] = n_chunks;
  }
}

// Backward work items.  A tile with n isects becomes ceil(n / L) items
// (tile, k): the full-length chunks go to `full`, the shorter tails to `tail`
// (the backward runs all full chunks first, so the longest items start
// first).  One lane per tile; one atomic per wave and list on the counters
// n_items[0..1], which the packed-gradient memset has zeroed.
__global__ void __launch_bounds__(256)
chunk_items_kernel(int n_tiles, const int32_t *__restrict__ offsets, int64_t n_isects,
                   const int64_t *__restrict__ n_dev, int L,
                   int2 *__restrict__ full, int2 *__restrict__ tail,
                   int32_t *__restrict__ n_items) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int nf = 0, nt = 0;
  if (t < n_tiles) {
    const int64_t e = tile_end(offsets, t, n_tiles, n_dev, n_isects);
    const int64_t n = e - offsets[t];
    nf = (int)(n / L);
    nt = (n % L) != 0;
  }
  int xf = nf, xt = nt;  // inclusive wave scans
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int yf = __shfl_up(xf, o, 64), yt = __shfl_up(xt, o, 64);
    if (lane >= o) {
      xf += yf;
      xt += yt;
    }
  }
  int bf = 0, bt = 0;
  if (lane == 63) {
    bf = xf ? atomicAdd(&n_items[0], xf) : 0;
    bt = xt ? atomicAdd(&n_items[1], xt) : 0;
  }
  bf = __shfl(bf, 63, 64) + xf - nf;
  bt = __shfl(bt, 63, 64) + xt - nt;
  for (int k = 0; k < nf; ++k) full[bf + k] = make_int2(t, k);
  if (nt) tail[bt] = make_int2(t, nf);
}

}  // namespace r16

// ---- Knobs.  Each is read from the environment on first use and then held
// in its global, which the setters below overwrite.
constexpr int kUnread = INT32_MIN;
static int g_chunk = kUnread, g_fwd_split = kUnread, g_split_div = kUnread,
           g_split_chunk = kUnread, g_dbg = kUnread;

static int knob(int &g, const char *name, int dflt, bool empty_is_unset = false) {
  if (g == kUnread) {
    const char *e = getenv(name);
    g = (e && !(empty_is_unset && !*e)) ? atoi(e) : dflt;
  }
  return g;
}

int dbg_flags() { return knob(g_dbg, "GSPLAT_HIP_DBG", 0); }

// Chunk length in isects for the chunked backward (multiple of 64; 0 turns
// chunking off).  GSPLAT_HIP_CHUNK overrides it for experiments.  256: at M2
// the two-pixel backward took 0.47 ms against 0.51 (512) and 0.61 (1024) on
// one box, for +6 us of chunk-state stores in the forward (tools/ab_chunk.sh).
int chunk_len() {
  const int x = knob(g_chunk, "GSPLAT_HIP_CHUNK", 256);
  return x <= 0 ? 0 : ((x + 63) / 64) * 64;
}

// Split heavy tiles in the forward (fwd_plan_kernel, "Split heavy tiles"):
// a tile with more isects than the threshold is rendered as parallel chunks
// of split_chunk() isects, concurrently with the other tiles, so that it no
// longer runs alone for the end of the launch.  Mode
// (GSPLAT_HIP_FWD_SPLIT / gsplat_hip_debug_set_fwd_split): unset, empty or
// < 0 = adaptive, threshold max(2048, n_isects / GSPLAT_HIP_FWD_SPLIT_DIV) --
// a tile longer than that fraction of all isects outlasts the rest of the
// launch (at M3 the heaviest, 21 k-isect tile ran 415 us against 250 us for
// 99 % of the waves) -- decided per tile on the device, so a render without
// such a tile runs the plain forward; > 0 = that fixed threshold; 0 = off.
static int fwd_split_mode() {
  return std::max(-1, knob(g_fwd_split, "GSPLAT_HIP_FWD_SPLIT", -1, true));
}

static int split_div() {
  const int x = knob(g_split_div, "GSPLAT_HIP_FWD_SPLIT_DIV", 550);
  return x > 0 ? x : 550;
}

static int64_t split_threshold(int64_t n_isects) {
  const int m = fwd_split_mode();
  if (m > 0) return m;
  return std::max<int64_t>(2048, n_isects / split_div());
}

// Isects per chunk of a split tile (GSPLAT_HIP_FWD_SPLIT_CHUNK, default
// 1024), a multiple of the backward's chunk length.
static int split_chunk() {
  const int x = knob(g_split_chunk, "GSPLAT_HIP_FWD_SPLIT_CHUNK", 1024), L = chunk_len();
  return L > 0 ? std::max(L, (x + L - 1) / L * L) : 0;
}

// ---- The forward's state: [chunk slots (L > 0): n_isects / L + 1 slots of
// 256 x (1 + D) floats][tile order (use_order)][split area (split_capable)].
static int64_t align256(int64_t x) { return (x + 255) / 256 * 256; }

int64_t chunk_slot_bytes(int D, int64_t n_isects) {
  const int L = chunk_len();
  if (L == 0 || n_isects <= 0) return 0;
  return (n_isects / L + 1) * (r16::kTS * r16::kTS * (1 + D)) * (int64_t)sizeof(float);
}

static bool use_order(int n_tiles, int64_t n_isects) {
  return n_isects > 0 && n_tiles > 0 && n_tiles <= 16384;
}

// XCD-grouped forward order (tile_order_grouped_kernel), the default for the
// unsplit forward; GSPLAT_HIP_DBG bit 4 restores the per-tile order.
// Measured (profiles/r6/xcd/, alternating bench runs, rocprofv3 counters of
// the forward): M2 forward 0.1622 / 0.1622 against 0.1655 / 0.1649 ms, L2 hit
// rate 0.618 -> 0.713, fetched bytes -27 %; M3 with the split off 0.605 /
// 0.603 against 0.608 / 0.608 ms, hit 0.451 -> 0.522, fetched -15 %.
static int order_slots(int C, int tw, int th) {
  return 32 * ((r16::order_groups(C, tw, th) + 7) / 8);
}
static bool grouped_order(int C, int tw, int th) {
  const int64_t n_tiles = (int64_t)C * tw * th;
  return !(dbg_flags() & 16) && r16::order_groups(C, tw, th) <= 8192 &&
         order_slots(C, tw, th) <= 2 * n_tiles + 64;
}

static int64_t order_bytes(int n_tiles, int64_t n_isects) {
  // room for the grouped order's slots too (32 ceil(groups / 8) <= 2 n_tiles
  // + 64 for any grid)
  return use_order(n_tiles, n_isects) ? align256(4 * (2 * (int64_t)n_tiles + 64)) : 0;
}

// The state has room for the split forward whenever it can run; which tiles
// split is decided per render on the device (fwd_plan_kernel).
static bool split_capable(int n_tiles, int64_t n_isects) {
  return fwd_split_mode() != 0 && chunk_len() > 0 && use_order(n_tiles, n_isects);
}

// The split area: [hdr 64 B][chunks int2 x (n_tiles + n_isects/SL + 1)][prod
// f32 x (n_isects/L + 1) x 256, by boundary slot][pflag i32 x (n_isects/L + 1)
// x 4][ctr i32 x (n_tiles + n_isects/SL + 1)][cout f32 x (n_tiles +
// n_isects/SL + 1) x 256 x (2 + D)], each part 256-B aligned (chunks: sum
// over split tiles of ceil(n / SL) <= n_tiles + n_isects / SL).
struct SplitLayout {
  int64_t hdr, fitems, prod, pflag, ctr, cout, bytes;
};

static SplitLayout split_layout(int D, int n_tiles, int64_t n_isects) {
  SplitLayout l{};
  if (!split_capable(n_tiles, n_isects)) return l;
  const int64_t nc = n_isects / chunk_len() + 1, ns = n_isects / split_chunk() + 1;
  const int64_t px = r16::kTS * r16::kTS;
  l.hdr = 0;
  l.fitems = 256;
  l.prod = l.fitems + align256(8 * ((int64_t)n_tiles + ns));
  l.pflag = l.prod + align256(4 * nc * px);
  l.ctr = l.pflag + align256(16 * nc);
  l.cout = l.ctr + align256(4 * ((int64_t)n_tiles + ns));
  l.bytes = l.cout + align256(4 * ((int64_t)n_tiles + ns) * px * (2 + D));
  return l;
}

int64_t rasterize16_fwd_state_bytes(int D, int n_tiles, int64_t n_isects) {
  return chunk_slot_bytes(D, n_isects) + order_bytes(n_tiles, n_isects) +
         split_layout(D, n_tiles, n_isects).bytes;
}

// Largest tile of the most recent dispatch-order kernel, written by the
// kernel into mapped pinned host memory (no copy, no sync).
static int32_t *g_stat_host = nullptr, *g_stat_dev = nullptr;

static int32_t *stat_dev() {
  if (!g_stat_host) {
    if (hipHostMalloc((void **)&g_stat_host, 64, hipHostMallocMapped) != hipSuccess) {
      g_stat_host = nullptr;
      return nullptr;
    }
    g_stat_host[0] = 0;
    if (hipHostGetDevicePointer((void **)&g_stat_dev, g_stat_host, 0) != hipSuccess)
      g_stat_dev = nullptr;
  }
  return g_stat_dev;
}

// Launch the split-capable forward?  Fixed threshold: always; adaptive: when
// an earlier render's largest tile exceeded this render's threshold (tiles
// are similar from one training step to the next).  Which tiles split is
// then decided on the device from this render's tiles (fwd_plan_kernel); a
// wrong guess costs speed only: an unsplit heavy tile, or the split-capable
// kernel's lower occupancy with nothing to split.  A captured step keeps the
// choice of its capture.
// The trainer takes the decision out of this heuristic: from its first
// render it sets a fixed threshold (always the split-capable forward) or 0
// (never) with gsplat_hip_set_fwd_split_threshold (Trainer._tune_split), so
// every render of a run -- eager or captured -- takes the same variant with
// the same threshold.
static bool use_split_now(int n_tiles, int64_t n_isects) {
  if (!split_capable(n_tiles, n_isects)) return false;
  if (fwd_split_mode() > 0) return true;
  stat_dev();
  const int32_t prev = g_stat_host ? *(volatile int32_t *)g_stat_host : 0;
  return prev > split_threshold(n_isects);
}

// State whose tile order gsplat_hip_rasterize_prepare already queued (so the
// forward call does not launch the order kernel again); cleared by the
// forward that consumes it.  Same host thread, same stream.
static thread_local const void *g_prepared_state = nullptr;
static thread_local bool g_prepared_split = false;  // the split decision of that preparation

static void launch_order(int C, int tw, int th, const int32_t *offsets, int64_t n_isects,
                         const int64_t *n_dev, int32_t *order, hipStream_t st,
                         char *split_base, int D) {
  const int n_tiles = C * tw * th;
  int32_t *max_out = split_capable(n_tiles, n_isects) ? stat_dev() : nullptr;
  if (split_base) {
    const SplitLayout l = split_layout(D, n_tiles, n_isects);
    hipLaunchKernelGGL(r16::fwd_plan_kernel, dim3(1), dim3(1024), 0, st, n_tiles, offsets,
                       n_isects, n_dev, split_chunk(), chunk_len(),
                       (int)std::min<int64_t>(split_threshold(n_isects), INT32_MAX),
                       reinterpret_cast<int32_t *>(split_base + l.hdr), order,
                       reinterpret_cast<int2 *>(split_base + l.fitems),
                       reinterpret_cast<int32_t *>(split_base + l.pflag),
                       reinterpret_cast<int32_t *>(split_base + l.ctr), max_out);
  } else if (grouped_order(C, tw, th)) {
    hipLaunchKernelGGL(r16::tile_order_grouped_kernel, dim3(1), dim3(1024), 0, st, C, tw, th,
                       offsets, n_isects, n_dev, order, max_out);
  } else {
    hipLaunchKernelGGL(r16::tile_order_kernel, dim3(1), dim3(1024), 0, st, n_tiles, offsets,
                       n_isects, n_dev, order, max_out);
  }
}

int rasterize16_prepare(int D, int C, int tw, int th, const int32_t *offsets, int64_t n_isects,
                        const int64_t *n_isects_dev, void *state, int64_t state_bytes,
                        hipStream_t st) {
  const int n_tiles = C * tw * th;
  g_prepared_state = nullptr;
  if (!state || !use_order(n_tiles, n_isects)) return 0;
  GS_REQUIRE(state_bytes >= rasterize16_fwd_state_bytes(D, n_tiles, n_isects),
             "rasterize_prepare: state too small");
  char *base = reinterpret_cast<char *>(state) + chunk_slot_bytes(D, n_isects);
  int32_t *order = reinterpret_cast<int32_t *>(base);
  const bool split = chunk_slot_bytes(D, n_isects) > 0 && use_split_now(n_tiles, n_isects);
  launch_order(C, tw, th, offsets, n_isects, n_isects_dev, order, st,
               split ? base + order_bytes(n_tiles, n_isects) : nullptr, D);
  GS_CHECK_LAUNCH("rasterize_prepare");
  g_prepared_state = state;
  g_prepared_split = split;
  return 0;
}

int plan_forward(r16::Args &a, int D, void *state, int64_t state_bytes, hipStream_t st,
                 FwdLaunch &launch) {
  const int64_t need = rasterize16_fwd_state_bytes(D, a.n_tiles, a.n_isects);
  GS_REQUIRE(state_bytes == 0 || state_bytes >= need,
             "rasterize_fwd: state of %lld bytes needed, %lld given", (long long)need,
             (long long)state_bytes);
  char *base = reinterpret_cast<char *>(state);
  const int64_t slots = chunk_slot_bytes(D, a.n_isects);
  a.L = chunk_len();
  a.state = (state && slots > 0) ? reinterpret_cast<float *>(state) : nullptr;
  a.order = (state && use_order(a.n_tiles, a.n_isects))
                ? reinterpret_cast<int32_t *>(base + slots) : nullptr;
  const bool prepared = state == g_prepared_state;
  const bool split = prepared ? g_prepared_split : use_split_now(a.n_tiles, a.n_isects);
  char *split_base = nullptr;
  if (a.order && a.state && split) {
    split_base = base + slots + order_bytes(a.n_tiles, a.n_isects);
    const SplitLayout l = split_layout(D, a.n_tiles, a.n_isects);
    a.n_whole = reinterpret_cast<const int32_t *>(split_base + l.hdr);
    a.n_chunks = a.n_whole + 1;
    a.fitems = reinterpret_cast<const int2 *>(split_base + l.fitems);
    a.prod = reinterpret_cast<float *>(split_base + l.prod);
    a.pflag = reinterpret_cast<int32_t *>(split_base + l.pflag);
    a.ctr = reinterpret_cast<int32_t *>(split_base + l.ctr);
    a.cout = reinterpret_cast<float *>(split_base + l.cout);
    a.SL = split_chunk();
  }
  if (a.order && !prepared)
    launch_order(a.C, a.tw, a.th, a.offsets, a.n_isects, a.n_dev, const_cast<int32_t *>(a.order),
                 st, split_base, D);
  g_prepared_state = nullptr;
  launch.split = split_base != nullptr;
  if (launch.split) {
    // the split tiles' chunks and the other tiles in one launch; the grid is
    // an upper bound (the plan's counts are on the device; surplus
    // workgroups exit)
    const int64_t nc = std::min<int64_t>(
        (int64_t)a.n_tiles + a.n_isects / a.SL + 1,
        a.n_isects / a.SL + a.n_isects / std::max<int64_t>(1, split_threshold(a.n_isects)) + 1);
    const int64_t nw = ((int64_t)a.n_tiles + 8 * r16::kItemRun - 1) / (8 * r16::kItemRun) *
                       (8 * r16::kItemRun);  // whole rounds of the XCD runs
    launch.grid = (unsigned)(nw + nc);
  } else {
    launch.grid = (a.order && grouped_order(a.C, a.tw, a.th)) ? order_slots(a.C, a.tw, a.th)
                                                              : a.n_tiles;
  }
  return 0;
}

// ---- The backward's workspace: [packed gradient rows][item counters 256 B]
// [work items int2 x n_items_bound: the full chunks' list, then the tails'].
size_t packed_bytes(int D, bool absgrad, int64_t G) {
  const int F = D + 6 + (absgrad ? 2 : 0);
  return (((size_t)sizeof(float) * ((F + 15) / 16) * 16 * G + 255) / 256) * 256;
}

int64_t n_items_bound(int n_tiles, int64_t n_isects) {
  const int L = chunk_len();
  const int64_t n = L ? (int64_t)n_tiles + n_isects / L + 1 : (int64_t)n_tiles;
  const int64_t q = 8 * r16::kItemRun;  // whole rounds of the XCD-aware item order
  return (n + q - 1) / q * q;
}

int64_t rasterize16_bwd_workspace(int64_t G, int D, bool absgrad, int n_tiles, int64_t n_isects) {
  int64_t b = (int64_t)packed_bytes(D, absgrad, G);
  if (chunk_len()) b += 256 + (int64_t)sizeof(int2) * n_items_bound(n_tiles, n_isects);
  return b;
}

int64_t plan_backward(r16::Args &a, char *items_base, hipStream_t st) {
  a.n_items = reinterpret_cast<int32_t *>(items_base);
  a.items = reinterpret_cast<int2 *>(items_base + 256);
  a.items_tail = a.items + (a.n_isects / a.L + 1);
  hipLaunchKernelGGL(r16::chunk_items_kernel, dim3((unsigned)((a.n_tiles + 255) / 256)),
                     dim3(256), 0, st, a.n_tiles, a.offsets, a.n_isects, a.n_dev, a.L,
                     const_cast<int2 *>(a.items), const_cast<int2 *>(a.items_tail),
                     const_cast<int32_t *>(a.n_items));
  return n_items_bound(a.n_tiles, a.n_isects);
}

}  // namespace gs

extern "C" int gsplat_hip_set_fwd_split_div(int div) {
  const int old = gs::split_div();
  gs::g_split_div = div > 0 ? div : gs::kUnread;
  return old;
}

extern "C" int gsplat_hip_set_fwd_split_threshold(int isects) {
  const int old = gs::fwd_split_mode();
  gs::g_fwd_split = isects < 0 ? -1 : isects;
  return old;
}

extern "C" int64_t gsplat_hip_fwd_split_threshold(int64_t n_isects) {
  return gs::fwd_split_mode() == 0 ? -1 : gs::split_threshold(n_isects);
}

extern "C" int gsplat_hip_debug_set_fwd_split(int isects) {
  return gsplat_hip_set_fwd_split_threshold(isects);
}

extern "C" int gsplat_hip_debug_set_flags(int flags) {
  const int old = gs::dbg_flags();
  gs::g_dbg = flags;
  return old;
}

extern "C" int gsplat_hip_debug_set_chunk(int isects) {
  gs::g_chunk = std::max(isects, 0);
  return gs::chunk_len();
}

