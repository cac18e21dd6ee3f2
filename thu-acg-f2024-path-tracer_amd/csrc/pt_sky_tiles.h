// The sure-sky tile test: can ANY camera ray of an 8x8 pixel tile enter one of the world's boxes? A tile for which the
// answer is a proven "no" is rendered by k_sky (pt_k_sky.hip) without ever entering the path pool; every other tile takes the wavefront.
// One function, compiled for the host (pt_sky_tiles, the CPU tests) and for the device (k_sky_classify), plain f64 + - * and comparisons.
// The same plane tests, read per box, also find the SHORT tiles of the short-path pass (sky_tile_class below): tiles whose
// camera rays can enter only boxes of entries that pass shades itself.
//
// The ray set of a tile (generate_ray, pt_dev_geom.h, perspective projection). With R = dof_right, U = dof_up (the basis times the lens radius):
//   origins   o = center + R px + U py,  px^2 + py^2 <= 1                                     (the lens disk; `center` itself when R = U = 0)
//   targets   T = pixel00 + pixel_dv (row + bx) + pixel_du (col + by),  bx^2 + by^2 <= blur^2   (rows and columns of the tile, clipped to the image)
//   ray       x(t) = o + t d,  t >= 0,  d = (T - o) / |T - o|
//
// The test, and why it is conservative:
//   1. Bounds. The disk of the lens lies in the square |px|, |py| <= 1; the targets lie in the parallelogram fy in [r0 - g, r1 + g],
//      fx in [c0 - g, c1 + g] with g = |blur| + 1/2 (the half pixel keeps the parallelogram from collapsing where a ragged edge leaves a
//      tile one row or column of pixels). pixel_du is parallel to R and pixel_dv to U (Camera::init builds both from `right` and `up`), so
//      T - o ranges over a parallelogram Q in the plane forward . q = -focal_length whose corners are q_k = T_k - center + sx_k R + sy_k U:
//      T_k a corner of the target parallelogram and (sx_k, sy_k) the signs that push it OUTWARDS (the sign of pixel_du . R for the corner of
//      larger fx, its opposite for the other; the same with pixel_dv . U). Every ray direction is a positive multiple of a point of Q, that is
//      a non-negative combination of q_0 .. q_3.
//   2. Side planes. n_k = q_k x q_{k+1}, negated if need be so that the two other corners have n_k . q_j < 0 (a plane for which that cannot be
//      had — a degenerate Q, a non-finite camera — is dropped: it clears nothing). Then n_k . q_j <= 0 for all four corners, hence
//      n_k . d <= 0 for every direction of the tile, and with c_k = max over the four lens corners of n_k . o every point of every ray has
//      n_k . x = n_k . o + t n_k . d <= c_k.
//   3. Fixed planes. For any normal n with n . q_j <= 0 at all four corners the same holds: n . x <= max over the lens corners of n . o.
//      Seven such normals are tried: `forward` (the lens plane; Q lies in forward . q = -focal_length < 0) and the six axis directions
//      +-x, +-y, +-z. The axis planes are what clears a box no frustum plane can: a ground slab below a camera whose tile looks upwards is
//      cut by every side plane somewhere behind or beside the camera, but lies wholly below the lens when no direction of the tile descends.
//   4. A box is CLEARED when for one of the eleven planes all eight of its corners p have n . p > c + margin: the box, the convex hull of its
//      corners, then lies strictly on the side no ray point reaches. The tile is sure sky when every box is cleared.
//   5. Margin: 1e-9 (|c| + |n| extent), extent = the largest |coordinate| among the boxes and the lens corners. The exact statement above is
//      about real arithmetic; the ray the kernels trace is the f64 rounding of it (sample location, origin, difference, normalisation:
//      a relative 1e-15 of the direction, so an absolute 1e-15 |n| extent in n . x at any point inside the scene's extent), and n_k, c_k and
//      n . p here are rounded the same way. 1e-9 covers both by six orders of magnitude. A NaN or an infinity anywhere makes a
//      comparison false or the margin infinite: nothing is cleared.
//   6. A lens corner inside or on a box: for every plane the box's corners p have min n . p <= n . o <= c for that corner o (a point of
//      the convex hull), so no plane clears the box — a camera inside or touching a box clears no tile.
// Primitives lie inside their entry's box (the boxes the top-level BVH was built from), so a ray that enters no box hits nothing: K2 would
// report a miss for it, and K3 would add the environment in its direction — what k_sky adds.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PT_SKY_HD __host__ __device__ inline
#else
#define PT_SKY_HD inline
#endif

namespace pt {

// At most this many boxes (a bit per box in sky_tile_is_clear). A world with more entries is tested against its ONE box, their union:
// the test is one thread per tile walking every box.
constexpr uint32_t SKY_MAX_BOXES = 64;

struct SkyCam {
    double center[3], forward[3], pixel00[3], pixel_du[3], pixel_dv[3], dof_right[3], dof_up[3];
    double blur_strength;
    double extent;            // the largest |coordinate| among the boxes and the lens corners (sky_extent)
    uint32_t width, height;
};

// Where box b's bit stands in a reach mask the device keeps (k_sky_classify): the place of entry b in the flat top level's loop
struct ReachOrder {
    uint8_t at[SKY_MAX_BOXES];
};

PT_SKY_HD double sky_abs(double x) { return x < 0.0 ? -x : x; }
PT_SKY_HD double sky_dot(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// `extent` of SkyCam for these boxes (six doubles each: lo.xyz, hi.xyz)
PT_SKY_HD double sky_extent(const SkyCam& c, uint32_t n_boxes, const double* boxes6) {
    double e = 0.0;
    for (uint32_t i = 0; i < 6 * n_boxes; ++i) {
        const double a = sky_abs(boxes6[i]);
        if (!(a <= e)) e = a;   // (a NaN becomes the extent: the margin is then NaN and nothing is cleared)
    }
    for (int i = 0; i < 3; ++i) {
        const double a = sky_abs(c.center[i]) + sky_abs(c.dof_right[i]) + sky_abs(c.dof_up[i]);
        if (!(a <= e)) e = a;
    }
    return e;
}

// The boxes the tile test could NOT clear for tile (ty, tx), bit b = box b: some ray generate_ray can produce for a pixel of the tile, some
// sample, may enter box b; every box whose bit is 0 is entered by none (the proof above). All ones where nothing can be said.
PT_SKY_HD unsigned long long sky_tile_uncleared(const SkyCam& c, uint32_t ty, uint32_t tx, uint32_t n_boxes, const double* boxes6) {
    if (n_boxes == 0u) return 0ull;
    if (n_boxes > SKY_MAX_BOXES) return ~0ull;
    const uint32_t r0 = ty * 8u, c0 = tx * 8u;
    if (r0 >= c.height || c0 >= c.width) return ~0ull;
    const uint32_t r1 = r0 + 7u < c.height ? r0 + 7u : c.height - 1u, c1 = c0 + 7u < c.width ? c0 + 7u : c.width - 1u;
    const double g = sky_abs(c.blur_strength) + 0.5;
    const double fy[2] = {(double)r0 - g, (double)r1 + g}, fx[2] = {(double)c0 - g, (double)c1 + g};
    // the outward lens signs of the high-fx and the high-fy corners
    const double sxh = sky_dot(c.pixel_du, c.dof_right) >= 0.0 ? 1.0 : -1.0, syh = sky_dot(c.pixel_dv, c.dof_up) >= 0.0 ? 1.0 : -1.0;
    // the corners of Q in cyclic order: (fy0, fx0), (fy0, fx1), (fy1, fx1), (fy1, fx0)
    double q[4][3];
    for (int k = 0; k < 4; ++k) {
        const int iy = k >> 1, ix = (k ^ (k >> 1)) & 1;
        const double sx = ix ? sxh : -sxh, sy = iy ? syh : -syh;
        for (int a = 0; a < 3; ++a)
            q[k][a] = ((c.pixel00[a] + c.pixel_dv[a] * fy[iy]) + c.pixel_du[a] * fx[ix]) - c.center[a] + (c.dof_right[a] * sx + c.dof_up[a] * sy);
    }
    double lens[4][3];
    for (int k = 0; k < 4; ++k)
        for (int a = 0; a < 3; ++a) lens[k][a] = c.center[a] + (c.dof_right[a] * ((k & 1) ? 1.0 : -1.0) + c.dof_up[a] * ((k & 2) ? 1.0 : -1.0));
    // the eleven planes, one after the other; bit b of `todo`: box b is not cleared yet
    unsigned long long todo = n_boxes >= 64u ? ~0ull : (1ull << n_boxes) - 1ull;
    for (int k = 0; k < 11 && todo != 0ull; ++k) {
        double n[3] = {0.0, 0.0, 0.0};
        bool ok = true;
        if (k < 4) {   // a side plane
            const double* a = q[k];
            const double* b = q[(k + 1) & 3];
            n[0] = a[1] * b[2] - a[2] * b[1];
            n[1] = a[2] * b[0] - a[0] * b[2];
            n[2] = a[0] * b[1] - a[1] * b[0];
            if (sky_dot(n, q[(k + 2) & 3]) + sky_dot(n, q[(k + 3) & 3]) > 0.0)
                for (int i = 0; i < 3; ++i) n[i] = -n[i];
            ok = sky_dot(n, q[(k + 2) & 3]) < 0.0 && sky_dot(n, q[(k + 3) & 3]) < 0.0;
        } else {       // the lens plane, then the six axis planes
            if (k == 4) for (int i = 0; i < 3; ++i) n[i] = c.forward[i];
            else n[(k - 5) >> 1] = ((k - 5) & 1) ? 1.0 : -1.0;
            for (int j = 0; j < 4; ++j) ok = ok && sky_dot(n, q[j]) <= 0.0;
        }
        double off = sky_dot(n, lens[0]);
        for (int j = 1; j < 4; ++j) {
            const double v = sky_dot(n, lens[j]);
            if (!(v <= off)) off = v;
        }
        const double len = sky_abs(n[0]) + sky_abs(n[1]) + sky_abs(n[2]);   // >= |n|
        const double margin = 1e-9 * (sky_abs(off) + len * c.extent);
        if (!(ok && len > 0.0 && margin >= 0.0 && margin < 1.7976931348623157e308)) continue;   // (a NaN drops the plane)
        for (uint32_t b = 0; b < n_boxes; ++b) {
            if (!((todo >> b) & 1ull)) continue;
            const double* bx = boxes6 + 6 * (size_t)b;
            bool outside = true;
            for (int j = 0; j < 8 && outside; ++j) {
                const double p[3] = {bx[(j & 1) ? 3 : 0], bx[(j & 2) ? 4 : 1], bx[(j & 4) ? 5 : 2]};
                outside = sky_dot(n, p) > off + margin;
            }
            if (outside) todo &= ~(1ull << b);
        }
    }
    return todo;
}
// true: no ray generate_ray can produce for any pixel of tile (ty, tx), any sample, enters any of the boxes.
PT_SKY_HD bool sky_tile_is_clear(const SkyCam& c, uint32_t ty, uint32_t tx, uint32_t n_boxes, const double* boxes6) {
    return sky_tile_uncleared(c, ty, tx, n_boxes, boxes6) == 0ull;
}
// The REACH mask of a tile: sky_tile_uncleared's answer, or all ones wherever the test says nothing — a tile outside the
// image, more boxes than the cap, a NaN or an infinity among the boxes or in the camera (sky_extent is then not finite), the lens's centre or a corner of it inside
// or on a box (point 6 above: that box is never cleared; the mask then names every box, so that a reader sees at once that nothing was
// said). A 0 bit is the proof above: no camera ray of the tile enters that box. The mask is 0 exactly for the sure-sky tiles.
PT_SKY_HD bool sky_tile_says_nothing(const SkyCam& c, uint32_t ty, uint32_t tx, uint32_t n_boxes, const double* boxes6) {
    if (n_boxes > SKY_MAX_BOXES || ty * 8u >= c.height || tx * 8u >= c.width || !(c.extent < 1.7976931348623157e308)) return true;
    for (uint32_t i = 0; i < 6 * n_boxes; ++i)
        if (!(boxes6[i] - boxes6[i] == 0.0)) return true;   // (sky_extent may have lost a NaN behind a later, finite coordinate)
    for (int k = 0; k < 5; ++k) {   // the lens's centre and its four corners
        double o[3];
        for (int a = 0; a < 3; ++a) o[a] = k == 4 ? c.center[a] : c.center[a] + (c.dof_right[a] * ((k & 1) ? 1.0 : -1.0) + c.dof_up[a] * ((k & 2) ? 1.0 : -1.0));
        for (uint32_t b = 0; b < n_boxes; ++b) {
            const double* bx = boxes6 + 6 * (size_t)b;
            if (bx[0] <= o[0] && o[0] <= bx[3] && bx[1] <= o[1] && o[1] <= bx[4] && bx[2] <= o[2] && o[2] <= bx[5]) return true;
        }
    }
    return false;
}
PT_SKY_HD unsigned long long sky_tile_reach(const SkyCam& c, uint32_t ty, uint32_t tx, uint32_t n_boxes, const double* boxes6) {
    if (n_boxes == 0u) return 0ull;
    return sky_tile_says_nothing(c, ty, tx, n_boxes, boxes6) ? ~0ull : sky_tile_uncleared(c, ty, tx, n_boxes, boxes6);
}
// The three kinds of tile. SURE SKY: every box is cleared. SHORT: every box that is NOT cleared is flagged in `shadeable`
// (bit b = box b: the box of an entry the short-path pass can shade, pt_flatten.cpp) — a camera ray of the tile hits such an entry or nothing.
// WAVEFRONT: everything else, and every tile about which nothing can be said (a tile outside the image, more boxes than the cap, a NaN or an
// infinity among the boxes or in the camera: sky_extent is then not finite). Only where the pass pays depends on this; no result does.
enum SkyTileClass : uint8_t { SKY_TILE_WAVEFRONT = 0, SKY_TILE_SKY = 1, SKY_TILE_SHORT = 2,
                              SKY_TILE_TAKEN = 3 };   // TAKEN: never this test's answer: a wavefront tile the short-path pass takes by its measured yield (k_short_select)
// (`todo`: sky_tile_uncleared's answer for the tile, which the caller has)
PT_SKY_HD uint8_t sky_tile_class_of(const SkyCam& c, uint32_t ty, uint32_t tx, uint32_t n_boxes, const double* boxes6, unsigned long long shadeable, unsigned long long todo) {
    if (n_boxes > SKY_MAX_BOXES || ty * 8u >= c.height || tx * 8u >= c.width) return SKY_TILE_WAVEFRONT;
    if (todo == 0ull) return SKY_TILE_SKY;
    if (!(c.extent < 1.7976931348623157e308) || (todo & ~shadeable) != 0ull) return SKY_TILE_WAVEFRONT;
    for (uint32_t b = 0; b < n_boxes; ++b)   // (a box with a NaN or an infinity is never cleared: flagged or not, it makes no tile short)
        for (int i = 0; i < 6 && ((todo >> b) & 1ull); ++i)
            if (!(boxes6[6 * (size_t)b + i] - boxes6[6 * (size_t)b + i] == 0.0)) return SKY_TILE_WAVEFRONT;
    return SKY_TILE_SHORT;
}
PT_SKY_HD uint8_t sky_tile_class(const SkyCam& c, uint32_t ty, uint32_t tx, uint32_t n_boxes, const double* boxes6, unsigned long long shadeable) {
    if (n_boxes > SKY_MAX_BOXES || ty * 8u >= c.height || tx * 8u >= c.width) return SKY_TILE_WAVEFRONT;
    return sky_tile_class_of(c, ty, tx, n_boxes, boxes6, shadeable, sky_tile_uncleared(c, ty, tx, n_boxes, boxes6));
}

}  // namespace pt
