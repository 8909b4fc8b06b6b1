// Lock-free union-find on parent words, shared by the ocean mask and the basin codes (include/ogg_hip.h, "Ocean mask" and "Basin
// codes"): the tile-local form on LDS words (workgroup scope) and the global form on device memory (agent scope).  A link puts the
// larger root under the smaller by an atomicMin, retried; parents only ever decrease along a chain, so no cycle can form, every
// retry is lock-free and no workgroup ever waits for another.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// ---- tile-local labelling in LDS ---------------------------------------------------------------------------------
__device__ inline int lds_find(int* lab, int x) {
    for (;;) {
        const int p = __hip_atomic_load(&lab[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p == x) return x;
        x = p;
    }
}

__device__ inline void lds_unite(int* lab, int a, int b) {
    a = lds_find(lab, a);
    b = lds_find(lab, b);
    while (a != b) {
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(&lab[a], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old == a) return;   // a linked under b
        a = lds_find(lab, old);   // a was linked elsewhere meanwhile (now under min(old, b)): join old's set and b's
        b = lds_find(lab, b);
    }
}

// ---- global parents ----------------------------------------------------------------------------------------------
// Other workgroups write parent words while a merge launch runs, so every read of one is an agent-scope relaxed atomic load (a plain
// load may return a stale line of another XCD's L2).
__device__ inline int glb_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ inline int glb_find(const int* par, int x) {
    for (;;) {
        const int p = glb_load(&par[x]);
        if (p == x) return x;
        x = p;
    }
}

// find with path halving: x's parent becomes its grandparent (an ancestor in the same set, of a smaller index: parents keep
// decreasing along every chain, so no cycle can form).  Used by the flatten launches, where only one thread per tile-local component
// walks: halving by every cell would put millions of atomics on the few words near a large component's root.
__device__ inline int glb_find_halving(int* par, int x) {
    for (;;) {
        const int p = glb_load(&par[x]);
        if (p == x) return x;
        const int gp = glb_load(&par[p]);
        if (gp == p) return p;
        __hip_atomic_fetch_min(&par[x], gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = gp;
    }
}

__device__ inline void glb_unite(int* par, int a, int b) {
    a = glb_find(par, a);
    b = glb_find(par, b);
    while (a != b) {
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(&par[a], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) return;
        a = glb_find(par, old);
        b = glb_find(par, b);
    }
}

}  // namespace
