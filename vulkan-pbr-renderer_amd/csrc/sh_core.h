// sh_core.h -- the nine-coefficient spherical-harmonic (SH9) form of an environment cube's diffuse lighting (K17),
// written once for the device kernels of k_sh.hip and for a host compiler: plain scalar C++, all arithmetic in double.
//
// Projection: coef[k][c] = sum over the texels of one cube level of L_c * Y_k(d) * domega, c = R, G, B (alpha is ignored); the fp32
// texel is widened exactly, products and sums are double.  Layout double[27], index 3 k + c.
//   d       the normalised face vector of the texel centre, faces as face_texel_dir of pbr_device.h
//   domega  the EXACT solid angle of the texel (not the centre approximation): with A(x, y) = atan2(x y, sqrt(x^2 + y^2 + 1)) and the
//           corner coordinates e_i = 2 i / n - 1,  domega = A(e_ix, e_iy) - A(e_ix, e_iy+1) - A(e_ix+1, e_iy) + A(e_ix+1, e_iy+1);
//           the six faces sum to 4 pi
//   Y_k     the real SH basis without Condon-Shortley phase (Ramamoorthi & Hanrahan 2001), k = 0 .. 8:
//           1, y, z, x, xy, yz, 3 z^2 - 1, xz, x^2 - y^2 times their constants, evaluated in double from the closed forms
// Irradiance, in the normalisation of the reference's gen_irradiance_map.glsl:84-97 (E / (2 pi): a constant environment c gives c / 2):
//   out_c(d) = sum_k a_k coef[k][c] Y_k(d),  a = {1/2, 1/3, 1/3, 1/3, 1/8, 1/8, 1/8, 1/8, 1/8},
// evaluated in double and rounded once to fp32 by the caller.  There is NO clamp: under a strong sun the nine-term series rings and
// the irradiance of directions facing away from it may be negative.
#pragma once
#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SH_FN __host__ __device__ __forceinline__
#else
#define SH_FN static inline
#endif

#define SH_PI 3.14159265358979323846

// e_i = 2 i / n - 1, as one correctly rounded quotient (2 i - n is exact)
SH_FN double sh_corner(int i, int n) { return (double)(2 * i - n) / (double)n; }
// centre coordinate of texel i: (2 i + 1 - n) / n
SH_FN double sh_centre(int i, int n) { return (double)(2 * i + 1 - n) / (double)n; }

SH_FN double sh_area(double x, double y) { return atan2(x * y, sqrt((x * x + y * y) + 1.0)); }
// domega from the four corner values, in the order every implementation keeps: a00 = A(e_ix, e_iy), a01 = A(e_ix, e_iy+1),
// a10 = A(e_ix+1, e_iy), a11 = A(e_ix+1, e_iy+1)
SH_FN double sh_solid_angle_of(double a00, double a01, double a10, double a11) { return ((a00 - a01) - a10) + a11; }
SH_FN double sh_solid_angle(int n, int ix, int iy) {
    const double x0 = sh_corner(ix, n), x1 = sh_corner(ix + 1, n), y0 = sh_corner(iy, n), y1 = sh_corner(iy + 1, n);
    return sh_solid_angle_of(sh_area(x0, y0), sh_area(x0, y1), sh_area(x1, y0), sh_area(x1, y1));
}

// 1 / |(1, sc, tc)|: the same for the six faces of one (ix, iy)
SH_FN double sh_inv_len(double sc, double tc) { return 1.0 / sqrt((sc * sc + tc * tc) + 1.0); }
// normalised direction of face `face` at centre coordinates (sc, tc); inv = sh_inv_len(sc, tc)
SH_FN void sh_face_dir(int face, double sc, double tc, double inv, double d[3]) {
    double x, y, z;
    switch (face) {
    case 0: x = 1.0; y = -tc; z = -sc; break;
    case 1: x = -1.0; y = -tc; z = sc; break;
    case 2: x = sc; y = 1.0; z = tc; break;
    case 3: x = sc; y = -1.0; z = -tc; break;
    case 4: x = sc; y = -tc; z = 1.0; break;
    default: x = -sc; y = -tc; z = -1.0; break;
    }
    d[0] = x * inv; d[1] = y * inv; d[2] = z * inv;
}

SH_FN void sh_basis(const double d[3], double Y[9]) {
    const double c0 = sqrt(1.0 / (4.0 * SH_PI)), c1 = sqrt(3.0 / (4.0 * SH_PI)), c2 = sqrt(15.0 / (4.0 * SH_PI));
    const double c20 = sqrt(5.0 / (16.0 * SH_PI)), c22 = sqrt(15.0 / (16.0 * SH_PI));
    const double x = d[0], y = d[1], z = d[2];
    Y[0] = c0;
    Y[1] = c1 * y; Y[2] = c1 * z; Y[3] = c1 * x;
    Y[4] = c2 * (x * y); Y[5] = c2 * (y * z);
    Y[6] = c20 * (3.0 * (z * z) - 1.0);
    Y[7] = c2 * (x * z);
    Y[8] = c22 * (x * x - y * y);
}

// acc[3 k + c] += L_c * (Y_k * domega)
SH_FN void sh_accumulate(double acc[27], const float rgb[3], const double Y[9], double domega) {
    for (int k = 0; k < 9; ++k) {
        const double w = Y[k] * domega;
        for (int c = 0; c < 3; ++c) acc[3 * k + c] = fma((double)rgb[c], w, acc[3 * k + c]);
    }
}

// out_c = sum_k (a_k coef[3 k + c]) Y_k(d), k ascending
SH_FN void sh_irradiance(const double coef[27], const double d[3], double out[3]) {
    const double a[9] = {1.0 / 2.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 8.0, 1.0 / 8.0, 1.0 / 8.0, 1.0 / 8.0, 1.0 / 8.0};
    double Y[9];
    sh_basis(d, Y);
    for (int c = 0; c < 3; ++c) {
        double s = 0.0;
        for (int k = 0; k < 9; ++k) s = s + (a[k] * coef[3 * k + c]) * Y[k];
        out[c] = s;
    }
}

// Host-order reference loops over rows [y0, y1) of faces [face0, face1) of one level (float RGBA [6][n][n]); the kernels add the same
// terms in another order.
SH_FN void sh_project_level(const float* level, int n, int face0, int face1, int y0, int y1, double out[27]) {
    for (int i = 0; i < 27; ++i) out[i] = 0.0;
    for (int f = face0; f < face1; ++f)
        for (int iy = y0; iy < y1; ++iy)
            for (int ix = 0; ix < n; ++ix) {
                const double sc = sh_centre(ix, n), tc = sh_centre(iy, n);
                double d[3], Y[9];
                sh_face_dir(f, sc, tc, sh_inv_len(sc, tc), d);
                sh_basis(d, Y);
                sh_accumulate(out, level + 4 * (((size_t)f * n + iy) * n + ix), Y, sh_solid_angle(n, ix, iy));
            }
}
SH_FN void sh_irradiance_texel(const double coef[27], int size, int face, int ix, int iy, float rgba[4]) {
    const double sc = sh_centre(ix, size), tc = sh_centre(iy, size);
    double d[3], e[3];
    sh_face_dir(face, sc, tc, sh_inv_len(sc, tc), d);
    sh_irradiance(coef, d, e);
    rgba[0] = (float)e[0]; rgba[1] = (float)e[1]; rgba[2] = (float)e[2]; rgba[3] = 0.0f;
}
