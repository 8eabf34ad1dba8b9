// panorama_core.h -- the direction of a pixel of a lat-long (equirectangular, 2:1 or any other extent) panorama (K20),
// written once for the device kernel of k_panorama.hip and for the host code that fills its tables and answers
// GPUX_PanoramaDirections.
//
// Pixel (x, y) of a w x h panorama looks along
//   phi   = ((2 x + 1) / w - 1) pi            longitude of the pixel centre, -pi .. pi
//   theta = (2 y + 1) / (2 h) pi              colatitude of the pixel centre: row 0 is next to +Z (the world is Z-up)
//   d     = (sin theta cos phi, sin theta sin phi, cos theta)
// the inverse of K6's u = atan2(d.y, d.x) / (2 pi) + 1/2, v = acos(d.z) / pi (k_equirect.hip) at u = (x + 1/2) / w, v = (y + 1/2) / h.
//
// The four trigonometric values are HOST values, in double, one pair per column and one per row (pano_column / pano_row): host and
// device must pick the same taps of the cube, and two libms need not agree in the last bit of a cosine, so the device takes them from
// a table instead of evaluating them.  pano_dir is what both sides run on a pair of table entries: the two products in double, each
// component rounded once to fp32.  d is not normalised again: the cube lookup is scale-free.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PANO_FN __host__ __device__ __forceinline__
#else
#define PANO_FN static inline
#endif

#define PANO_PI 3.14159265358979323846
#define PANO_MAX_EXTENT 16384

// one table entry per column: {cos phi, sin phi}; per row: {sin theta, cos theta}.  Host only.
static inline void pano_column(int x, int w, double cs[2]) {
    const double phi = ((double)(2 * x + 1) / (double)w - 1.0) * PANO_PI;
    cs[0] = cos(phi); cs[1] = sin(phi);
}
static inline void pano_row(int y, int h, double sc[2]) {
    const double theta = (double)(2 * y + 1) / (double)(2 * h) * PANO_PI;
    sc[0] = sin(theta); sc[1] = cos(theta);
}
// The table of a w x h panorama: 2 w doubles (columns) followed by 2 h doubles (rows).
static inline void pano_fill_table(int w, int h, double* table) {
    for (int x = 0; x < w; ++x) pano_column(x, w, table + 2 * x);
    for (int y = 0; y < h; ++y) pano_row(y, h, table + 2 * (w + y));
}

PANO_FN void pano_dir(const double col[2], const double row[2], float d[3]) {
    d[0] = (float)(row[0] * col[0]);
    d[1] = (float)(row[0] * col[1]);
    d[2] = (float)row[1];
}
