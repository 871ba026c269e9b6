// ordered_device.h -- the order-preserving compaction pieces that csrc/mesh_components.hip and csrc/mesh_simplify.hip share: the
// single-workgroup scan of per-workgroup counts and the destination of a flagged item.  No atomics: the same rows from launch to
// launch.  (Everything here sits in an anonymous namespace: each unit that includes it gets its own copy of the kernel.)
#pragma once
#include "common.h"

namespace {

constexpr int kOrderedBlock = 256;          // threads, and items per workgroup of the order-preserving passes
constexpr int kOrderedWaves = kOrderedBlock / scanerf::kWave;

// One workgroup: blocks [n] -> its exclusive sums in place, blocks[n] = *total = the sum.
constexpr int kScanThreads = 1024;
__global__ void __launch_bounds__(kScanThreads) k_scan(int *__restrict__ blocks, int n, long long *__restrict__ total)
{
    __shared__ int sums[kScanThreads];
    const int per = (n + kScanThreads - 1) / kScanThreads;
    const int lo = min(n, (int)threadIdx.x * per), hi = min(n, lo + per);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += blocks[i];
    sums[threadIdx.x] = s;
    __syncthreads();
    for (int off = 1; off < kScanThreads; off <<= 1) {          // inclusive scan of the threads' sums
        const int add = (int)threadIdx.x >= off ? sums[threadIdx.x - off] : 0;
        __syncthreads();
        sums[threadIdx.x] += add;
        __syncthreads();
    }
    int run = sums[threadIdx.x] - s;
    for (int i = lo; i < hi; ++i) {
        const int c = blocks[i];
        blocks[i] = run;
        run += c;
    }
    if (threadIdx.x == kScanThreads - 1) {
        blocks[n] = sums[threadIdx.x];
        *total = sums[threadIdx.x];
    }
}

// The destination of a flagged item: (flagged items of earlier workgroups) + (of earlier waves) + (of lower lanes).
__device__ __forceinline__ int destination(bool on, const int *__restrict__ blocks, int *part)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long ballot = __ballot(on);
    if (lane == 0) part[wv] = __popcll(ballot);
    __syncthreads();
    int dst = blocks[blockIdx.x];
    for (int w = 0; w < wv; ++w) dst += part[w];
    return dst + __popcll(ballot & ((1ull << lane) - 1ull));
}

// blocks[blockIdx.x] = the flagged items among the workgroup's kOrderedBlock items
__device__ __forceinline__ void count_flagged(bool on, int *__restrict__ blocks, int *part)
{
    const unsigned long long ballot = __ballot(on);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = __popcll(ballot);
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < kOrderedWaves; ++w) s += part[w];
        blocks[blockIdx.x] = s;
    }
}

}  // namespace
