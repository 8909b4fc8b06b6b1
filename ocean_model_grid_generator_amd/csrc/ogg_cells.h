// The topology of the model cells, shared by the runoff mapping, the distance to the coast and the remap fill (include/ogg_hip.h):
// the four face neighbours of a cell.  What a caller does with a neighbour that does not exist is its own rule.
#pragma once
#include "../../include/ogg_hip.h"

namespace {

struct CellTopo {
    long ny, nx;
    int periodic, fold;
};

// from the OGG_MASK_PERIODIC | OGG_MASK_FOLD flags of a parameter struct
inline CellTopo cell_topo(long ny, long nx, int topology) {
    return CellTopo{ny, nx, (topology & OGG_MASK_PERIODIC) ? 1 : 0, (topology & OGG_MASK_FOLD) ? 1 : 0};
}

// S, W, E, N of cell c (-1: none): the seam is crossed only on a periodic grid, and only the top row has a fold partner
__device__ inline void face_neighbours(const CellTopo& t, long c, long (&nb)[4]) {
    const long j = c / t.nx, i = c % t.nx;
    nb[0] = j > 0 ? c - t.nx : -1;
    nb[1] = i > 0 ? c - 1 : (t.periodic ? c + t.nx - 1 : -1);
    nb[2] = i < t.nx - 1 ? c + 1 : (t.periodic ? c - (t.nx - 1) : -1);
    nb[3] = j < t.ny - 1 ? c + t.nx : (t.fold ? j * t.nx + (t.nx - 1 - i) : -1);
}

}  // namespace
