// Connected components of the cells of a ny x nx plane under a per-cell class, shared by the ocean mask (one class: wet) and the
// basin codes (a class per rule of a pass) (include/ogg_hip.h, "Ocean mask" and "Basin codes").  Two cells are joined when they share
// a face and have the SAME class other than NONE; the periodic seam joins (j, nx - 1) ~ (j, 0) and the fold joins
// (ny - 1, i) ~ (ny - 1, nx - 1 - i).  Union-find in three launches (label_components), so the number of launches does not grow with a
// component's diameter (a serpentine channel is one component of millions of cells):
//
// label_tile            the body of the caller's tile kernel, one workgroup per tile of TW x th cells.  The kernel itself forms the
//                       classes in LDS (the classify loop stays in the kernel's own body: moved into a function of its own, the
//                       basin's box scan compiles to a longer inner loop); label_tile then runs a union-find in LDS over the faces
//                       inside the tile (link the larger root under the smaller by an LDS atomicMin, retried); every cell's parent
//                       becomes the GLOBAL index of its tile-local root, -1 for a cell of class NONE.  Row-major local indices map
//                       monotonically to global ones, so that root is the smallest global index of the tile-local component.  With
//                       MANY a tile without an eligible cell leaves after writing its parents.
// label_merge_kernel    one thread per face that crosses a tile edge, the periodic seam or the fold (Faces): the same union on the
//                       global parents, with agent-scope atomicMin links.  Other workgroups write parent words in this launch, so
//                       every read of one is an agent-scope relaxed atomic load (a plain load may return a stale line of another
//                       XCD's L2).  Parents only ever decrease, so there is no cycle; the retry is lock-free and no workgroup waits
//                       on another.
// label_flatten_kernel  its own launch (every link is in place): root[c] = find(c), the smallest index of the cell's component, -1
//                       for class NONE.  Inside a tile the cells follow their parents in LDS to a representative; only
//                       representatives walk the global chains (halving them as they go).  With COUNT, the cells per root too:
//                       counted per representative in LDS, then one atomicAdd per (tile, representative), so the world ocean does
//                       not serialise millions of atomics on one word.
//
// MANY: more than one class (the basin codes), a class byte per tile cell in LDS after the parents; most tiles of such a launch hold no
// eligible cell, which is what the early exits of tile and flatten are for.  One class (the ocean mask): the parents alone, no early
// exit, the cells per root.  The merge launch takes a predicate: __device__ bool operator()(const int* par, long a, long b) const, true
// if a and b have one class other than NONE (after the tile launch, class != NONE is par >= 0).
#pragma once
#include <hip/hip_runtime.h>

#include "ogg_blocks.h"
#include "ogg_common.h"

namespace {

constexpr int TW = 64;           // tile width: one wavefront across a tile row
constexpr int NT = 256;          // threads per workgroup
constexpr int TH_DEFAULT = 32;   // tile rows (OGG_MASK_TILE_ROWS, OGG_BASIN_TILE_ROWS)
constexpr int TH_MAX = 64;
constexpr int NONE = 255;        // the class of a cell that belongs to no component

static_assert(NT == BLOCKS_NT, "block_add sums over a workgroup of BLOCKS_NT threads");

struct Grid {
    long ny, nx;
    int th, nbx;   // tile rows, tiles across a row
};

struct Faces {
    long ny, nx;
    int th;
    long n_v, n_h, n_p, n_f;   // faces across vertical tile edges, horizontal tile edges, the seam, the fold
};

inline Grid label_grid(long ny, long nx, int th) { return Grid{ny, nx, th, (int)((nx + TW - 1) / TW)}; }

// topology: OGG_MASK_PERIODIC | OGG_MASK_FOLD.  A band one or two cells wide has no seam face that is not already a face (or the
// cell itself); the fold pairs i < nx - 1 - i, so the middle cell of an odd row, its own partner, has none.
inline Faces label_faces(const Grid& g, int topology) {
    Faces f{g.ny, g.nx, g.th, (long)(g.nbx - 1) * g.ny, ((g.ny + g.th - 1) / g.th - 1) * g.nx, 0, 0};
    if ((topology & OGG_MASK_PERIODIC) && g.nx > 2) f.n_p = g.ny;
    if (topology & OGG_MASK_FOLD) f.n_f = g.nx / 2;
    return f;
}

// ---- lock-free union-find on parent words: LDS words (workgroup scope), device memory (agent scope) ---------------
// A link puts the larger root under the smaller by an atomicMin, retried; parents only ever decrease along a chain, so no cycle can
// form, every retry is lock-free and no workgroup ever waits for another.
__device__ inline int lds_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__device__ inline int lds_find(int* lab, int x) {
    for (;;) {
        const int p = lds_load(&lab[x]);
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
// decreasing along every chain, so no cycle can form).  Used by the flatten launch, where only one thread per tile-local component
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

// ---- the tile-local labelling in LDS ---------------------------------------------------------------------------------
// lab: TW * th parents, lab[l] = l for a cell of a class, -1 for NONE and off the grid; with MANY then TW * th class bytes.  any: this
// thread met a cell of a class.  Every thread of the workgroup calls it, right after it has written its cells (the barrier is here).
template <bool MANY>
__device__ inline void label_tile(const Grid& g, long j0, long i0, int* lab, int any, int* par) {
    const int n = TW * g.th;
    const auto cls_of = [&](int l) {
        return MANY ? (int)reinterpret_cast<unsigned char*>(lab + n)[l] : (lds_load(&lab[l]) >= 0 ? 0 : NONE);
    };
    if (!MANY) {
        __syncthreads();
    } else if (__syncthreads_or(any) == 0) {   // nothing to label in this tile
        for (int l = threadIdx.x; l < n; l += NT) {
            const long j = j0 + l / TW, i = i0 + l % TW;
            if (j < g.ny && i < g.nx) par[j * g.nx + i] = -1;
        }
        return;
    }
    for (int l = threadIdx.x; l < n; l += NT) {
        const int k = cls_of(l);
        if (k == NONE) continue;
        const int tx = l % TW, ty = l / TW;
        if (tx + 1 < TW && cls_of(l + 1) == k) lds_unite(lab, l, l + 1);
        if (ty + 1 < g.th && cls_of(l + TW) == k) lds_unite(lab, l, l + TW);
    }
    __syncthreads();
    for (int l = threadIdx.x; l < n; l += NT) {
        const long j = j0 + l / TW, i = i0 + l % TW;
        if (j >= g.ny || i >= g.nx) continue;
        int p = -1;
        if (cls_of(l) != NONE) {
            const int r = lds_find(lab, l);
            p = (int)((j0 + r / TW) * g.nx + i0 + r % TW);
        }
        par[j * g.nx + i] = p;
    }
}

// ---- merge across tile edges, the seam and the fold ----------------------------------------------------------------
template <class P>
__global__ __launch_bounds__(NT) void label_merge_kernel(Faces f, P same, int* par) {
    const long total = f.n_v + f.n_h + f.n_p + f.n_f;
    for (long t = (long)blockIdx.x * NT + threadIdx.x; t < total; t += (long)gridDim.x * NT) {
        long a, b, u = t;
        if (u < f.n_v) {   // (j, i - 1) ~ (j, i), i = (k + 1) * TW
            const long k = u / f.ny, j = u % f.ny;
            a = j * f.nx + (k + 1) * TW - 1;
            b = a + 1;
        } else if ((u -= f.n_v) < f.n_h) {   // (j - 1, i) ~ (j, i), j = (k + 1) * th
            const long k = u / f.nx, i = u % f.nx;
            a = ((k + 1) * f.th - 1) * f.nx + i;
            b = a + f.nx;
        } else if ((u -= f.n_h) < f.n_p) {   // (j, nx - 1) ~ (j, 0)
            a = u * f.nx + f.nx - 1;
            b = u * f.nx;
        } else {   // (ny - 1, i) ~ (ny - 1, nx - 1 - i), i < nx - 1 - i
            u -= f.n_p;
            a = (f.ny - 1) * f.nx + u;
            b = (f.ny - 1) * f.nx + f.nx - 1 - u;
        }
        if (same(par, a, b)) glb_unite(par, (int)a, (int)b);   // class NONE stays -1
    }
}

// ---- flatten; with COUNT (one class) the cells per root, without it (MANY) the early exit ------------------------
// The tile's parents go to LDS; every cell follows them inside the tile to its representative (the first cell whose parent is
// itself or lies outside the tile).  Only the representatives walk the global chains; the other cells take their representative's
// root from LDS.
template <bool COUNT>
__global__ __launch_bounds__(NT) void label_flatten_kernel(Grid g, int* par, int* __restrict__ root, int* size) {
    extern __shared__ int sh[];
    const int n = TW * g.th;
    int* lp = sh;            // the parent of each tile cell as a tile-local index, -1 outside the tile, -2 for class NONE / off the grid
    int* rt = sh + n;        // the root of each representative
    int* cnt = sh + 2 * n;   // COUNT: cells per representative
    const long i0 = (long)(blockIdx.x % g.nbx) * TW, j0 = (long)(blockIdx.x / g.nbx) * g.th;
    int any = 0;
    for (int l = threadIdx.x; l < n; l += NT) {
        const long j = j0 + l / TW, i = i0 + l % TW;
        int v = -2;
        if (j < g.ny && i < g.nx) {
            const int p = glb_load(&par[j * g.nx + i]);   // (another tile's walk may halve it: any value read is an ancestor)
            if (p >= 0) {
                const long pj = p / g.nx, pi = p % g.nx;
                v = (pj >= j0 && pj < j0 + g.th && pi >= i0 && pi < i0 + TW) ? (int)((pj - j0) * TW + (pi - i0)) : -1;
                if (v == l) v = -1;   // a root: its own representative
            }
        }
        lp[l] = v;
        if (COUNT) cnt[l] = 0;
        any |= v != -2;
    }
    if (COUNT) {
        __syncthreads();
    } else if (__syncthreads_or(any) == 0) {   // no component in this tile
        for (int l = threadIdx.x; l < n; l += NT) {
            const long j = j0 + l / TW, i = i0 + l % TW;
            if (j < g.ny && i < g.nx) root[j * g.nx + i] = -1;
        }
        return;
    }
    for (int l = threadIdx.x; l < n; l += NT)
        if (lp[l] == -1) rt[l] = glb_find_halving(par, (int)((j0 + l / TW) * g.nx + i0 + l % TW));
    __syncthreads();
    for (int l = threadIdx.x; l < n; l += NT) {
        const long j = j0 + l / TW, i = i0 + l % TW;
        if (j >= g.ny || i >= g.nx) continue;
        int r = -1;
        if (lp[l] != -2) {
            int q = l;
            while (lp[q] >= 0) q = lp[q];   // in-tile parents have smaller local indices: this ends
            r = rt[q];
            if (COUNT) atomicAdd(&cnt[q], 1);
        }
        root[j * g.nx + i] = r;
    }
    if (COUNT) {
        __syncthreads();
        for (int l = threadIdx.x; l < n; l += NT)
            if (cnt[l] > 0) atomicAdd(&size[rt[l]], cnt[l]);
    }
}

// tile, merge (if there is a face to merge across), flatten, on the caller's stream: root[c] for every cell, and with COUNT the cells
// of every root added to size[root] (zeroed by the caller).  par: ny * nx words of workspace.  tile(g, tiles) launches the caller's tile
// kernel, one workgroup per tile.
template <bool COUNT, class T, class P>
int label_components(long ny, long nx, int th, int topology, const T& tile, const P& same, int* par, int* root, int* size,
                     hipStream_t st) {
    const Grid g = label_grid(ny, nx, th);
    const Faces f = label_faces(g, topology);
    const unsigned tiles = (unsigned)(g.nbx * ((ny + th - 1) / th));
    const long faces = f.n_v + f.n_h + f.n_p + f.n_f;
    tile(g, tiles);
    OGG_LAUNCH_CHECK();
    if (faces > 0) {
        label_merge_kernel<<<ogg::grid_for<NT>(faces, 4096), NT, 0, st>>>(f, same, par);
        OGG_LAUNCH_CHECK();
    }
    label_flatten_kernel<COUNT><<<tiles, NT, (COUNT ? 3 : 2) * TW * th * sizeof(int), st>>>(g, par, root, size);
    OGG_LAUNCH_CHECK();
    return OGG_OK;
}

}  // namespace
