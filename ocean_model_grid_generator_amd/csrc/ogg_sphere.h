// Nearest-point searches on the sphere, shared by the runoff mapping, the distance to the coast, the basin codes and the ocean mask's
// seeds (include/ogg_hip.h): the unit vector of a point and the squared chordal distance in its one rounding order, its bits as a
// sort key, the nearest-so-far under that key with its pruning margin, and the centre point of a model cell.  (The counting sort of
// unit vectors into cubes: ogg_sphere_bins.h.)
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr double SPHERE_D = 0.017453292519943295;   // pi / 180

__device__ inline void unit(double lon, double lat, double* u) {
    const double cl = cos(lat * SPHERE_D);
    u[0] = cl * cos(lon * SPHERE_D);
    u[1] = cl * sin(lon * SPHERE_D);
    u[2] = sin(lat * SPHERE_D);
}

__device__ inline double dist2(double ax, double ay, double az, double bx, double by, double bz) {
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ inline unsigned long long bits_of(double v) { return (unsigned long long)__double_as_longlong(v); }

// On every comparison of two computed squared distances.  A difference of two doubles, a product and a square root are each correctly
// rounded, so a computed distance is within a few 2^-53 of its value RELATIVELY, however small: the margin covers the rounding of a
// computed d2, and of a lower bound compared with it, a million times over.
constexpr double MARGIN = 1.0 + 1e-12;

// The nearest candidate so far by the key (d2 bits, cell): the smaller bits of the squared chord (positive doubles order as their
// bits), then the smaller cell, so the order in which candidates are met does not matter.  A search starts from {ULLONG_MAX, INT_MAX}.
struct Nearest {
    unsigned long long bits;
    int cell;
    __device__ inline void offer(unsigned long long b, int c) { if (b < bits || (b == bits && c < cell)) bits = b, cell = c; }
    __device__ inline bool found() const { return cell != INT_MAX; }
    __device__ inline double d2() const { return __longlong_as_double((long long)bits); }
    // is the squared lower bound lb2 of some candidates beyond the best, margin included?  (Never before anything was found.)
    __device__ inline bool beyond(double lb2) const { return found() && lb2 > d2() * MARGIN; }
};

// the centre of model cell (j, i), or of cell c of rows of nx cells, on a supergrid of row stride ld: point (2 j + 1, 2 i + 1)
__device__ inline long centre_ji(long j, long i, long ld) { return (2 * j + 1) * ld + 2 * i + 1; }
__device__ inline long centre_point(long c, long nx, long ld) { return centre_ji(c / nx, c % nx, ld); }

// its unit vector
__device__ inline void centre_unit(const double* x, const double* y, long c, long nx, long ld, double* u) {
    const long k = centre_point(c, nx, ld);
    unit(x[k], y[k], u);
}

}  // namespace
