// Workgroup reductions and scans shared by the logits row kernels (region.hip, sampling.hip, logprobs.hip,
// logits_edit.hip) and by argmax_kernel (elementwise.hip).  Each is the ONE definition of a step whose result several
// entry points promise to agree on bit for bit: an integer or compare reduction, whose result does not depend on the
// order of evaluation, or a floating-point reduction whose order is part of the contract written at its callers.
#pragma once
#include "md_common.hpp"

// ---------------------------------------------------------------------------
// argmax over (value, index): the greater value wins, equal values go to the lower index, a NaN never wins.
__device__ __forceinline__ void argmax_take(float& best, int& bi, float v, int i) {
  if (v > best || (v == best && i < bi)) {
    best = v;
    bi = i;
  }
}

// The workgroup's winner from every thread's own (best, bi), which start at (-inf, 0x7fffffff) and take the thread's
// share in ascending index order: a 6-level xor butterfly per wave, one partial per wave in sv / si [WAVES], a fold by
// thread 0.  The return value is thread 0's alone: the index, or 0 where nothing won (bi >= n: an all-NaN row selects
// nothing, and the caller uses the result as a table index).  One barrier, after the partials are stored.
template <int WAVES>
__device__ __forceinline__ int block_argmax(float best, int bi, int n, float* sv, int* si) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) argmax_take(best, bi, __shfl_xor(best, o, 64), __shfl_xor(bi, o, 64));
  if ((threadIdx.x & 63) == 0) {
    sv[threadIdx.x >> 6] = best;
    si[threadIdx.x >> 6] = bi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < WAVES; ++w) argmax_take(best, bi, sv[w], si[w]);
    if (bi >= n) bi = 0;
  }
  return bi;
}

// ---------------------------------------------------------------------------
// The 16 wave partials of a 1024-thread workgroup (token_logprobs_kernel's steps 2 -> 3): lane 0 of a wave stores the
// wave's reduced value; after a barrier of the caller's, every thread folds the 16 by a 4-level xor butterfly (offsets 8,
// 4, 2, 1: every 16 consecutive lanes hold the 16 partials), so all threads hold the same total.
template <class T>
__device__ __forceinline__ void wave_partial_store(T v, T* red) {
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
}
template <class T>
__device__ __forceinline__ T fold16_sum(const T* red) {
  T v = red[threadIdx.x & 15];
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float fold16_max(const float* red) {
  float v = red[threadIdx.x & 15];
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// ---------------------------------------------------------------------------
// Inclusive prefix of v over a wave's lanes, by __shfl_up (integers: exact).
template <class T>
__device__ __forceinline__ T wave_inclusive_scan(T v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T up = __shfl_up(v, o, 64);
    if ((int)(threadIdx.x & 63) >= o) v += up;
  }
  return v;
}

// Inclusive prefix of v over the THREADS threads of the workgroup: Hillis-Steele over scan[THREADS], doubling offsets, so
// the order of a float prefix's additions is a function of the thread's index alone.  scan[] keeps the prefixes
// afterwards.  The caller orders its last reads of scan[] before the call; ends in a barrier.
template <int THREADS, class T>
__device__ __forceinline__ T block_inclusive_scan(T v, T* scan) {
  const int tid = threadIdx.x;
  scan[tid] = v;
  __syncthreads();
  for (int off = 1; off < THREADS; off <<= 1) {
    const T add = (tid >= off) ? scan[tid - off] : T(0);
    __syncthreads();
    scan[tid] += add;
    __syncthreads();
  }
  return scan[tid];
}

// ---------------------------------------------------------------------------
// the id row r's logits lose (-1: none): suppress_id, on every row or on the rows that suppress_rows marks
__device__ __forceinline__ int row_suppress(int suppress_id, const int32_t* __restrict__ suppress_rows, int r) {
  return (suppress_id >= 0 && (suppress_rows == nullptr || suppress_rows[r] != 0)) ? suppress_id : -1;
}

// the slot of row r's per-sequence state: slots[r], or slot0 + r without a table
__device__ __forceinline__ int state_slot(const int32_t* __restrict__ slots, int slot0, int r) {
  return slots ? slots[r] : slot0 + r;
}
