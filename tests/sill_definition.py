"""The definition of the sill depths (include/ogg_hip.h, "Sill depths") in numpy and plain Python, twice over: a heap-based widest
path from the seeds (sill_heap) and Kruskal in descending weight with union-find (sill_kruskal).  Both give b; regions, gates and
counts follow from b (finish).  Nothing here is shared with the package: the tests hold the device result EQUAL to this."""
import heapq

import numpy as np

SEED = 1 << 30
PERIODIC, FOLD = 1, 2
COUNT_FIELDS = ("rounds", "n_clamped", "n_bad_seeds", "n_connected", "n_cut_off", "n_regions", "n_gate_faces")


def bits_for(wu, wv):
    """the smallest bits (1 .. 30) that holds the largest weight"""
    top = max(int(np.max(wu, initial=0)), int(np.max(wv, initial=0)), 1)
    return min(max(top.bit_length(), 1), 30)


def passages(ny, nx, wu, wv, topology, bits):
    """[(a, b, w, faces)], faces the [(kind, row, column, swapped)] the passage's gate code is written to, and n_clamped"""
    wu, wv = np.asarray(wu, dtype=np.int64).reshape(ny, nx + 1), np.asarray(wv, dtype=np.int64).reshape(ny + 1, nx)
    wmax = (1 << bits) - 1
    clamped = [0]

    def rd(w):
        c = min(max(int(w), 0), wmax)
        clamped[0] += c != int(w)
        return c
    out = []
    for j in range(ny):
        for i in range(1, nx):
            out.append((j * nx + i - 1, j * nx + i, rd(wu[j, i]), [("u", j, i, False)]))
    for j in range(1, ny):
        for i in range(nx):
            out.append(((j - 1) * nx + i, j * nx + i, rd(wv[j, i]), [("v", j, i, False)]))
    if (topology & PERIODIC) and nx > 2:
        for j in range(ny):
            out.append((j * nx + nx - 1, j * nx, min(rd(wu[j, 0]), rd(wu[j, nx])), [("u", j, 0, False), ("u", j, nx, False)]))
    if topology & FOLD:
        for i in range(nx):
            k = nx - 1 - i
            if i < k:
                out.append(((ny - 1) * nx + i, (ny - 1) * nx + k, min(rd(wv[ny, i]), rd(wv[ny, k])),
                            [("v", ny, i, False), ("v", ny, k, True)]))
    return out, clamped[0]


def _adjacency(n, ps):
    adj = [[] for _ in range(n)]
    for a, b, w, _ in ps:
        adj[a].append((b, w))
        adj[b].append((a, w))
    return adj


def good_seeds(n, seeds):
    s = [int(c) for c in seeds]
    return sorted(set(c for c in s if 0 <= c < n)), sum(1 for c in s if not 0 <= c < n)


def sill_heap(n, ps, seeds):
    """b by a widest-path search from all seeds at once (a max-heap on the bottleneck so far)"""
    b = np.zeros(n, dtype=np.int64)
    adj = _adjacency(n, ps)
    heap = []
    for c in seeds:
        b[c] = SEED
        heap.append((-SEED, c))
    heapq.heapify(heap)
    done = np.zeros(n, dtype=bool)
    while heap:
        v, c = heapq.heappop(heap)
        if done[c]:
            continue
        done[c] = True
        for q, w in adj[c]:
            t = min(-v, w)
            if not done[q] and b[q] != SEED and t > b[q]:
                b[q] = t
                heapq.heappush(heap, (-t, q))
    return b


def _find(par, x):
    while par[x] != x:
        par[x] = par[par[x]]
        x = par[x]
    return x


def sill_kruskal(n, ps, seeds):
    """b by adding the passages in descending weight: a set without a seed that meets a set with one at weight w has b = w"""
    par = list(range(n))
    members = [[c] for c in range(n)]
    seeded = [False] * n
    b = np.zeros(n, dtype=np.int64)
    for c in seeds:
        seeded[c] = True
        b[c] = SEED
    for a, q, w, _ in sorted(ps, key=lambda p: -p[2]):
        if w <= 0:
            break
        ra, rq = _find(par, a), _find(par, q)
        if ra == rq:
            continue
        if seeded[ra] != seeded[rq]:
            for c in members[rq if seeded[ra] else ra]:
                b[c] = w
        if len(members[ra]) < len(members[rq]):
            ra, rq = rq, ra
        par[rq] = ra
        members[ra] += members[rq]
        members[rq] = []
        seeded[ra] = seeded[ra] or seeded[rq]
    return b


def finish(ny, nx, ps, b, bits, n_clamped, n_bad):
    """region, gate_u, gate_v and the counts from b"""
    n = ny * nx
    par = list(range(n))
    for a, q, w, _ in ps:
        if b[a] == b[q] and 0 < b[a] < SEED and w >= b[a]:
            ra, rq = _find(par, a), _find(par, q)
            if ra != rq:
                par[max(ra, rq)] = min(ra, rq)
    region = np.array([-1 if b[c] == 0 else (c if b[c] == SEED else _find(par, c)) for c in range(n)], dtype=np.int32)
    gates = {"u": np.zeros((ny, nx + 1), dtype=np.uint8), "v": np.zeros((ny + 1, nx), dtype=np.uint8)}
    for a, q, w, faces in ps:
        code = 1 if 0 < b[a] == w < b[q] else (2 if 0 < b[q] == w < b[a] else 0)
        for kind, r, col, swapped in faces:
            gates[kind][r, col] = (3 - code) if (swapped and code) else code
    positive = np.zeros(n, dtype=bool)
    for a, q, w, _ in ps:
        if w > 0:
            positive[a] = positive[q] = True
    counts = {"rounds": bits, "n_clamped": n_clamped, "n_bad_seeds": n_bad, "n_connected": int(np.sum((b > 0) & (b < SEED))),
              "n_cut_off": int(np.sum((b == 0) & positive)), "n_regions": int(np.sum(region == np.arange(n))),
              "n_gate_faces": int(np.count_nonzero(gates["u"]) + np.count_nonzero(gates["v"]))}
    return region.reshape(ny, nx), gates["u"], gates["v"], counts


def sill(wu, wv, seeds, topology, bits=None, search=sill_heap):
    """the whole definition: a dict b (int32), region, gate_u, gate_v, counts, bits"""
    wu, wv = np.asarray(wu), np.asarray(wv)
    ny, nx = wu.shape[0], wv.shape[1]
    assert wu.shape == (ny, nx + 1) and wv.shape == (ny + 1, nx)
    if bits is None:
        bits = bits_for(wu, wv)
    ps, n_clamped = passages(ny, nx, wu, wv, topology, bits)
    good, n_bad = good_seeds(ny * nx, seeds)
    b = search(ny * nx, ps, good)
    region, gu, gv, counts = finish(ny, nx, ps, b, bits, n_clamped, n_bad)
    return {"b": b.astype(np.int32).reshape(ny, nx), "region": region, "gate_u": gu, "gate_v": gv, "counts": counts, "bits": bits}


# ---- the quantiser and the weights of the two modes (float64, as the package states them) ------------------------------
def quantise(d, quantum):
    d = np.asarray(d, dtype=np.float64)
    ok = np.isfinite(d) & (d != 1.0e20)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.clip(np.rint(np.where(ok, d, 0.0) / quantum), 0, (1 << 30) - 1)
    return np.where(ok, q, 0).astype(np.int64)


def cell_weights(qd, wet, topology):
    """cells mode: a face's weight is the smaller q(depth) of its two cells, 0 next to a cell that is not wet; the seam's and the
    fold's faces take their partner across the seam / fold, faces with one side only hold 0"""
    ny, nx = qd.shape
    q = np.where(wet != 0, qd, 0)
    wu = np.zeros((ny, nx + 1), dtype=np.int64)
    wv = np.zeros((ny + 1, nx), dtype=np.int64)
    wu[:, 1:nx] = np.minimum(q[:, :-1], q[:, 1:])
    wv[1:ny] = np.minimum(q[:-1], q[1:])
    if topology & PERIODIC:
        wu[:, 0] = wu[:, nx] = np.minimum(q[:, -1], q[:, 0])
    if topology & FOLD:
        wv[ny] = np.minimum(q[-1], q[-1, ::-1])
    return wu, wv


# ---- weights for the tests -------------------------------------------------------------------------------------------
def serpentine(ny=64, nx=66, shallow=None):
    """A channel one cell wide winding through ny x nx cells: rows 0, 2, 4, ... run the whole width, joined alternately at the east
    and the west end through one cell of the odd rows.  Weights descend along the channel from the seed (cell 0); every other face is
    0.  shallow: the index along the channel of one face made shallower than everything after it.  (wu, wv, seed, faces)"""
    path = []
    for r, j in enumerate(range(0, ny, 2)):
        cols = range(nx) if r % 2 == 0 else range(nx - 1, -1, -1)
        path += [(j, i) for i in cols]
        if j + 2 < ny:
            path.append((j + 1, nx - 1 if r % 2 == 0 else 0))
    wu = np.zeros((ny, nx + 1), dtype=np.int64)
    wv = np.zeros((ny + 1, nx), dtype=np.int64)
    m = len(path) - 1
    for k in range(m):
        (j0, i0), (j1, i1) = path[k], path[k + 1]
        w = 2 * (m - k) + 10
        if shallow is not None and k == shallow:
            w = 3
        if j0 == j1:
            wu[j0, max(i0, i1)] = w
        else:
            wv[max(j0, j1), i0] = w
    return wu, wv, 0, m
