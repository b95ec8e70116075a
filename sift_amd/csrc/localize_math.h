// Sub-pixel keypoint localisation (include/sift_hip.h, "sub-pixel localisation"): THE DEFINITION.  The HIP kernel
// (kernels_localize.hip) and the host checker (hostmath_capi.cpp: hostmath_localize) both compile this header, with
// -ffp-contract=off.  Plain IEEE double operations in the order written, one rounding each; NO fma and no libm call, so that a
// float64 restatement with the same operation order (tests/localize_ref.py) gives the same bits.  An extension: the reference
// solves for the offset in Sift::_eliminateEdgeResponses (sift.cpp:300-329) and throws it away.
//
// A stack is the L >= 3 DoG levels of one octave, w x h each; a keypoint is (x, y, i).  One step at a sample position with
// 1 <= x <= w - 2, 1 <= y <= h - 2, 1 <= i <= L - 2 fits the 3D quadratic through the 27 samples around it (Lowe 2004,
// section 4): gradient and Hessian by central differences, the offset of the vertex by the adjugate and the determinant.
// Sample (a, b, c), each in {-1, 0, 1}, is d(x + a, y + b, i + c) and lies at s[9 * (c + 1) + 3 * (b + 1) + (a + 1)].
//   converged   |ox| <= 0.5 and |oy| <= 0.5 and |os| <= 0.5
//   move        otherwise every axis steps by +1 where o > 0.5, by -1 where o < -0.5, else 0
//   the loop    step; converged -> OK; else if `max_moves` moves were made -> NOT_CONVERGED (the budget is asked first); else
//               if the new position leaves the ranges above -> LEFT_RANGE; else move, fetch, step again
// The keypoint's OWN position must lie in those ranges: localize_point fetches around it without asking.  The entries that take
// points from a caller refuse others (SIFT_HIP_EINVAL); the batch kernel, whose keypoints come from the extremum scan and are
// interior by construction, guards its loads all the same and gives such a point LEFT_RANGE, 0 moves and value +0.0f - the one
// record the host loop has no counterpart for.
#pragma once
#include <stdint.h>

#include "fdlibm_atan2f.h"   // SIFT_HD
#include "../../include/sift_hip.h"

namespace sift_hip {

constexpr int kLocalizeMaxMoves = 8;
constexpr int kLocalizeMove = 255;   // localize_step: not converged, not failed (never stored in a record)

SIFT_HD bool loc_finite(double v) { return v - v == 0.0; }   // false for a NaN and for both infinities
SIFT_HD bool loc_finite(float v) { return v - v == 0.0f; }

struct LocFit {
    double ox, oy, os;   // the offset of the vertex from the sample position
    double gx, gy, gs;   // the gradient there
    double d0;           // the centre sample
};

// One step.  SIFT_HIP_LOCALIZE_OK: converged; kLocalizeMove: the vertex lies in another sample's cell; else the final status.
SIFT_HD int localize_step(const float (&s)[27], LocFit& f) {
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 27; ++k) finite = finite && loc_finite(s[k]);
    if (!finite) return SIFT_HIP_LOCALIZE_NOT_FINITE;
#define SIFT_LOC_D(a, b, c) ((double)s[9 * ((c) + 1) + 3 * ((b) + 1) + ((a) + 1)])
    const double d0 = SIFT_LOC_D(0, 0, 0);
    const double gx = 0.5 * (SIFT_LOC_D(1, 0, 0) - SIFT_LOC_D(-1, 0, 0));
    const double gy = 0.5 * (SIFT_LOC_D(0, 1, 0) - SIFT_LOC_D(0, -1, 0));
    const double gs = 0.5 * (SIFT_LOC_D(0, 0, 1) - SIFT_LOC_D(0, 0, -1));
    const double hxx = (SIFT_LOC_D(1, 0, 0) + SIFT_LOC_D(-1, 0, 0)) - (d0 + d0);
    const double hyy = (SIFT_LOC_D(0, 1, 0) + SIFT_LOC_D(0, -1, 0)) - (d0 + d0);
    const double hss = (SIFT_LOC_D(0, 0, 1) + SIFT_LOC_D(0, 0, -1)) - (d0 + d0);
    const double hxy = 0.25 * ((SIFT_LOC_D(1, 1, 0) - SIFT_LOC_D(-1, 1, 0)) - (SIFT_LOC_D(1, -1, 0) - SIFT_LOC_D(-1, -1, 0)));
    const double hxs = 0.25 * ((SIFT_LOC_D(1, 0, 1) - SIFT_LOC_D(-1, 0, 1)) - (SIFT_LOC_D(1, 0, -1) - SIFT_LOC_D(-1, 0, -1)));
    const double hys = 0.25 * ((SIFT_LOC_D(0, 1, 1) - SIFT_LOC_D(0, -1, 1)) - (SIFT_LOC_D(0, 1, -1) - SIFT_LOC_D(0, -1, -1)));
#undef SIFT_LOC_D
    // the adjugate of the symmetric H = [hxx hxy hxs; hxy hyy hys; hxs hys hss], every entry p * q - r * s
    const double a00 = hyy * hss - hys * hys;
    const double a01 = hxs * hys - hxy * hss;
    const double a02 = hxy * hys - hxs * hyy;
    const double a11 = hxx * hss - hxs * hxs;
    const double a12 = hxy * hxs - hxx * hys;
    const double a22 = hxx * hyy - hxy * hxy;
    // cofactors along the first row, summed left to right: the minors are a00, -a01 and a02
    const double m1 = hxy * hss - hys * hxs;
    const double m2 = hxy * hys - hyy * hxs;
    const double det = (hxx * a00 - hxy * m1) + hxs * m2;
    if (det == 0.0 || !loc_finite(det)) return SIFT_HIP_LOCALIZE_SINGULAR;
    // off = -(adj(H) g) / det: one sum of three products in row order, negated, one division
    f.ox = -((a00 * gx + a01 * gy) + a02 * gs) / det;
    f.oy = -((a01 * gx + a11 * gy) + a12 * gs) / det;
    f.os = -((a02 * gx + a12 * gy) + a22 * gs) / det;
    f.gx = gx; f.gy = gy; f.gs = gs; f.d0 = d0;
    if (!(loc_finite(f.ox) && loc_finite(f.oy) && loc_finite(f.os))) return SIFT_HIP_LOCALIZE_NOT_FINITE;
    const bool cx = f.ox <= 0.5 && f.ox >= -0.5, cy = f.oy <= 0.5 && f.oy >= -0.5, cs = f.os <= 0.5 && f.os >= -0.5;
    return (cx && cy && cs) ? SIFT_HIP_LOCALIZE_OK : kLocalizeMove;
}

SIFT_HD int loc_move(double o) { return o > 0.5 ? 1 : (o < -0.5 ? -1 : 0); }
SIFT_HD bool loc_interior(int x, int y, int i, int w, int h, int L) { return x >= 1 && x <= w - 2 && y >= 1 && y <= h - 2 && i >= 1 && i <= L - 2; }

// After a step that asked for a move, with `moves` made so far: the status that ends the point, or kLocalizeMove with the
// position stepped.
SIFT_HD int localize_advance(const LocFit& f, int moves, int max_moves, int w, int h, int L, int& x, int& y, int& i) {
    if (moves >= max_moves) return SIFT_HIP_LOCALIZE_NOT_CONVERGED;
    const int nx = x + loc_move(f.ox), ny = y + loc_move(f.oy), ni = i + loc_move(f.os);
    if (!loc_interior(nx, ny, ni, w, h, L)) return SIFT_HIP_LOCALIZE_LEFT_RANGE;
    x = nx; y = ny; i = ni;
    return kLocalizeMove;
}

// the coordinate the gather builds without localisation: (float)(v << octave) * coord_scale
SIFT_HD float loc_plain_coord(uint32_t v, int octave, float coord_scale) { return (float)(v << octave) * coord_scale; }

// The record.  (kx, ky, ki): the keypoint's own position; (x, y, i): the final sample position; centre0: the centre sample at the
// keypoint's own position; coord_scale: 0.5f after a subpixel batch, else 1.0f (2^octave and it are exact factors).
SIFT_HD sift_hip_localized localize_record(int status, const LocFit& f, int kx, int ky, int ki, int x, int y, int i, int moves, int octave,
                                           float coord_scale, float centre0) {
    sift_hip_localized r;
    r.status = (uint8_t)status;
    r.moves = (uint8_t)moves;
    r.reserved = 0;
    if (status == SIFT_HIP_LOCALIZE_OK) {
        const double scale = (double)(1u << octave) * (double)coord_scale;
        r.x = (float)(((double)x + f.ox) * scale);
        r.y = (float)(((double)y + f.oy) * scale);
        r.dx = (float)f.ox; r.dy = (float)f.oy; r.ds = (float)f.os;
        r.value = (float)(f.d0 + 0.5 * ((f.gx * f.ox + f.gy * f.oy) + f.gs * f.os));
        r.mx = (int16_t)(x - kx); r.my = (int16_t)(y - ky); r.mi = (int8_t)(i - ki);
    } else {
        r.x = loc_plain_coord((uint32_t)kx, octave, coord_scale);
        r.y = loc_plain_coord((uint32_t)ky, octave, coord_scale);
        r.dx = r.dy = r.ds = 0.0f;
        r.value = centre0;
        r.mx = r.my = 0; r.mi = 0;
    }
    return r;
}

// The whole point, one after another: what the host loop runs.  fetch(x, y, i, s) fills the 27 samples around a position.
template <class Fetch>
inline sift_hip_localized localize_point(Fetch&& fetch, int w, int h, int L, int kx, int ky, int ki, int max_moves, int octave, float coord_scale) {
    float s[27];
    int x = kx, y = ky, i = ki, moves = 0, status;
    LocFit f{};
    fetch(x, y, i, s);
    const float centre0 = s[13];
    for (;;) {
        status = localize_step(s, f);
        if (status != kLocalizeMove) break;
        status = localize_advance(f, moves, max_moves, w, h, L, x, y, i);
        if (status != kLocalizeMove) break;
        ++moves;
        fetch(x, y, i, s);
    }
    return localize_record(status, f, kx, ky, ki, x, y, i, moves, octave, coord_scale, centre0);
}

}  // namespace sift_hip
