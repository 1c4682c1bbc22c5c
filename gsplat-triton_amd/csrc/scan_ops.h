// Integer prefix scans over a wave, a workgroup and an array (gfx950, wave64),
// shared by every counting pass: tile intersection, the supertile expansion,
// the LSD sort, the 16x16 rasterizer's plan, packed projection, densification,
// PLY rows and marching cubes.  Every scanned value is an
// integer, so the order of the additions never shows in a result.
//
// All of them take the lane from threadIdx.x: one-dimensional workgroups of
// whole waves, every lane of which reaches the call.
#pragma once

#include "common.h"

namespace gs {

// Inclusive scan over the wave's 64 lanes in lane order (Hillis-Steele).  Two
// values are scanned by two calls: the compiler interleaves the two chains.
template <class T>
GS_INLINE T wave_inclusive_scan(T x) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  return x;
}

// Exclusive scan of v over the workgroup's WAVES * 64 lanes in lane order;
// the workgroup's sum -> total (in every lane).  A wave scan, the waves' sums
// into wsum, ONE barrier, then every lane adds the sums of the waves before
// its own, and all of them for the total.
// wsum: the call ends without a barrier, so a caller that writes wsum again
// (a second scan, the next round of a loop) puts its own barrier in between.
template <int WAVES, class T>
GS_INLINE T block_exclusive_scan(T v, T (&wsum)[WAVES], T &total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const T x = wave_inclusive_scan(v);
  if (lane == 63) wsum[wid] = x;
  __syncthreads();
  T before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    before += w < wid ? wsum[w] : (T)0;
    all += wsum[w];
  }
  total = all;
  return before + x - v;
}

// The same scan with the waves' sums combined by thread 0 alone: two barriers
// and serial LDS traffic for the WAVES selects and adds in every lane.  Kept
// for packed_scan_kernel, whose rounds of int64 counts over 16 waves ran 15 %
// slower with the every-lane form.  Same wsum contract.
template <int WAVES, class T>
GS_INLINE T block_exclusive_scan_t0(T v, T (&wsum)[WAVES], T &total) {
  __shared__ T all;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const T x = wave_inclusive_scan(v);
  if (lane == 63) wsum[wid] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    T run = 0;
    for (int w = 0; w < WAVES; ++w) {
      const T t = wsum[w];
      wsum[w] = run;
      run += t;
    }
    all = run;
  }
  __syncthreads();
  total = all;
  return wsum[wid] + x - v;
}

// Exclusive scan of row[0, n) in place by ONE 1024-lane workgroup; returns the
// row's sum (in every lane).  A lane takes K consecutive elements per round,
// all its loads in flight before the first is used (a round covers 1024 K
// elements for one load latency), and the rounds chain through a carry.
// T0: the thread-0 combine above.  Ends with a barrier: wave_tot is free again
// on return.
template <class T, int K, bool T0 = false>
GS_INLINE T array_exclusive_scan(T *row, int64_t n, T (&wave_tot)[16]) {
  T carry = 0;  // identical in every lane
  for (int64_t base = 0; base < n; base += 1024 * K) {
    const int64_t i0 = base + (int64_t)threadIdx.x * K;
    T v[K], s = 0, all;
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = (i0 + k < n) ? row[i0 + k] : (T)0;
#pragma unroll
    for (int k = 0; k < K; ++k) s += v[k];
    T run = carry + (T0 ? block_exclusive_scan_t0(s, wave_tot, all)
                        : block_exclusive_scan(s, wave_tot, all));
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (i0 + k < n) row[i0 + k] = run;
      run += v[k];
    }
    carry += all;
    __syncthreads();
  }
  return carry;
}

}  // namespace gs
