// Workgroup building blocks shared by the analyses' translation units (ocean mask, remap, runoff, regrid, bilinear): the sum of a few
// counters over a workgroup with one atomic per block, the exclusive prefix over a workgroup, the missing-value test of a source
// field, and the three-kernel exclusive scan of a device array.  Nothing here depends on the launch geometry beyond the workgroup size.
#pragma once
#include <hip/hip_runtime.h>

#include "ogg_common.h"

namespace {

constexpr int BLOCKS_NT = 256;                      // threads per workgroup of every kernel that calls block_add / block_scan
constexpr int SCAN_PER = 8;                         // items per thread of the scan
constexpr int SCAN_CH = BLOCKS_NT * SCAN_PER;       // items per scan block

__device__ inline unsigned long long* ull(long long* p) { return reinterpret_cast<unsigned long long*>(p); }

// block sums of K counters: wavefront shuffles, then LDS, then one atomicAdd per block and non-zero counter (a counter word takes
// every block's add, so the adds per word are as few as the blocks)
template <int K>
__device__ inline void block_add(long long (&v)[K], long long* const (&dst)[K]) {
    __shared__ long long part[BLOCKS_NT / 64][K];
    for (int k = 0; k < K; ++k)
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < K; ++k) part[threadIdx.x / 64][k] = v[k];
    __syncthreads();
    if (threadIdx.x < K) {
        long long t = 0;
        for (int w = 0; w < BLOCKS_NT / 64; ++w) t += part[w][threadIdx.x];
        if (t) atomicAdd(ull(dst[threadIdx.x]), (unsigned long long)t);
    }
}

// exclusive prefix of v over the workgroup; *total the sum
__device__ inline long long block_scan(long long v, long long* total) {
    __shared__ long long wsum[BLOCKS_NT / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x / 64;
    long long incl = v;
    for (int o = 1; o < 64; o <<= 1) {
        const long long t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    long long base = 0, tot = 0;
    for (int k = 0; k < BLOCKS_NT / 64; ++k) {
        if (k < w) base += wsum[k];
        tot += wsum[k];
    }
    __syncthreads();
    *total = tot;
    return base + incl - v;
}

// a source value that is NaN or one of the field's nf (0 .. 2) fill values
template <typename T>
__device__ inline bool missing(T v, T f0, T f1, int nf) {
    return v != v || (nf > 0 && v == f0) || (nf > 1 && v == f1);
}

// ---- exclusive scan of a device array ------------------------------------------------------------------------------
// The total goes where the caller wants it, fixed at compile time (TAIL): behind the n prefixes, as entry n of an output of n + 1
// entries, or to a word of its own while the output has n entries.  (All three kernels are templates, so only the translation units
// that scan hold them.)

// bsum[b] = the sum of in over block b (SCAN_CH items)
template <typename T>
__global__ __launch_bounds__(BLOCKS_NT) void scan_count_kernel(const T* __restrict__ in, long n, long long* __restrict__ bsum) {
    const long b0 = (long)blockIdx.x * SCAN_CH;
    long long v = 0;
    for (int k = 0; k < SCAN_PER; ++k) {
        const long i = b0 + k * BLOCKS_NT + threadIdx.x;
        if (i < n) v += (long long)in[i];
    }
    long long tot;
    (void)block_scan(v, &tot);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// exclusive scan of the nb block sums in place (one workgroup); without TAIL, *total the sum
template <bool TAIL>
__global__ __launch_bounds__(BLOCKS_NT) void scan_blocks_kernel(long long* bsum, long nb, long long* total) {
    long long carry = 0;
    for (long base = 0; base < nb; base += BLOCKS_NT) {
        const long i = base + threadIdx.x;
        const long long v = i < nb ? bsum[i] : 0;
        long long tot;
        const long long ex = block_scan(v, &tot);
        if (i < nb) bsum[i] = carry + ex;
        carry += tot;
    }
    if (!TAIL && threadIdx.x == 0) *total = carry;
}

// out[i] = the sum of in[i'] for i' < i, for i < n (with TAIL: i <= n, out[n] the total); SCAN_PER consecutive items per thread, so
// the order is the index order
template <bool TAIL, typename T>
__global__ __launch_bounds__(BLOCKS_NT) void scan_write_kernel(const T* __restrict__ in, long n, const long long* __restrict__ bsum,
                                                               int* __restrict__ out) {
    const long i0 = (long)blockIdx.x * SCAN_CH + (long)threadIdx.x * SCAN_PER;
    long long v[SCAN_PER], s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_PER; ++k) {
        v[k] = i0 + k < n ? (long long)in[i0 + k] : 0;
        s += v[k];
    }
    long long tot;
    long long run = bsum[blockIdx.x] + block_scan(s, &tot);
#pragma unroll
    for (int k = 0; k < SCAN_PER; ++k) {
        if (i0 + k < n + (TAIL ? 1 : 0)) out[i0 + k] = (int)run;
        run += v[k];
    }
}

// out[i] = the exclusive prefix of the n items of in, for i < n; the total to out[n] (TAIL) or to *total (otherwise; total is not
// read with TAIL); bsum: one word of scratch per block of SCAN_CH entries of out
template <bool TAIL, typename T>
int exclusive_scan(const T* in, long n, long long* bsum, long long* total, int* out, hipStream_t st) {
    const long nb = (n + (TAIL ? 1 : 0) + SCAN_CH - 1) / SCAN_CH;
    scan_count_kernel<T><<<(unsigned)nb, BLOCKS_NT, 0, st>>>(in, n, bsum);
    OGG_LAUNCH_CHECK();
    scan_blocks_kernel<TAIL><<<1, BLOCKS_NT, 0, st>>>(bsum, nb, total);
    OGG_LAUNCH_CHECK();
    scan_write_kernel<TAIL, T><<<(unsigned)nb, BLOCKS_NT, 0, st>>>(in, n, bsum, out);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

}  // namespace
