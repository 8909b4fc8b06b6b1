// Device sort of unique 64-bit keys shared by the translation units that group a list by a key (runoff segments, the lat-lon regrid's
// transpose): runs of KEYSORT_NT keys sorted in LDS by the caller, then keysort_merge_kernel passes that merge runs of w keys in pairs.
// A key's slot is its place in its run plus the number of keys of the partner run below it (a binary search), so the keys must be
// unique; the cost is O(n log n) whatever the distribution of the keys.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int KEYSORT_NT = 256;   // keys per LDS-sorted run, threads per workgroup of the merge

// runs of w sorted keys merged in pairs: a key's slot is its place in its run plus the keys of the partner run below it
__global__ __launch_bounds__(KEYSORT_NT) void keysort_merge_kernel(const unsigned long long* __restrict__ in, long n, long w,
                                                                  unsigned long long* __restrict__ out) {
    for (long i = (long)blockIdx.x * KEYSORT_NT + threadIdx.x; i < n; i += (long)gridDim.x * KEYSORT_NT) {
        const unsigned long long key = in[i];
        const long r = i / w, rs = r * w;
        long lo = (r & 1) ? rs - w : rs + w;
        long hi = (r & 1) ? rs : (rs + 2 * w < n ? rs + 2 * w : n);
        const long p0 = lo;
        if (lo > n) lo = hi = n;
        while (lo < hi) {
            const long m = lo + (hi - lo) / 2;
            if (in[m] < key) lo = m + 1;
            else hi = m;
        }
        out[(r & ~1L) * w + (i - rs) + (lo - (p0 > n ? n : p0))] = key;
    }
}

// the number of merge passes after the LDS sort of runs of KEYSORT_NT keys, so which of two key buffers holds the sorted keys
inline int keysort_passes(long n) {
    int k = 0;
    for (long w = KEYSORT_NT; w < n; w *= 2) ++k;
    return k;
}

}  // namespace
