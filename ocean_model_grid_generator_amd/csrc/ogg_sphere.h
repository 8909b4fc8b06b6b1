// Nearest-point searches on the sphere, shared by the runoff mapping, the distance to the coast, the basin codes and the ocean mask's
// seeds (include/ogg_hip.h): the unit vector of a point and the squared chordal distance in its one rounding order, with its bits as
// a sort key.  (The counting sort of unit vectors into cubes: ogg_sphere_bins.h.)
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

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

__device__ inline unsigned long long bits_of(double v) {
    unsigned long long b;
    memcpy(&b, &v, 8);
    return b;
}

}  // namespace
