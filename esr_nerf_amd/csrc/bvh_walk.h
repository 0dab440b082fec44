// The walk of the surface's BVH (section T of include/esr_hip.h), shared by the kernels that cast a ray of their own: the
// nearest-hit / any-hit kernels of bvh.hip and the shadow segments of surflight.hip.  One lane walks one ray.
//
// No stack.  A lane holds its node, its depth and a TRAIL of one bit per level -- which child of that level's node it
// entered first (the one whose box the ray enters sooner).  Coming back up from a child it reads the parent link
// (2 parent + side), compares the side with the trail bit and either tests the other child or climbs on.  The tree is at
// most 63 + 31 levels deep (key bits + position bits), the trail is 128 bits in two registers: correct at every depth the
// build can produce, no LDS, no scratch.  What it costs against a stack: coming back to a node loads its record again
// (64 bytes, in L2) and tests the far child's box again.
// Nothing is pruned at equality (enter <= best) and equal t goes to the smaller face id, so the answer does not depend on
// the order of the walk.
//
// Arithmetic of a triangle test (binary64, contraction off, every operation rounded on its own, in this order):
//   e1 = b - a, e2 = c - a, p = d x e2, det = (e1.x p.x + e1.y p.y) + e1.z p.z, s = o - a, q = s x e1,
//   u = ((s.x p.x + s.y p.y) + s.z p.z) / det, v = ((d.x q.x + d.y q.y) + d.z q.z) / det,
//   t = ((e2.x q.x + e2.y q.y) + e2.z q.z) / det, w = (1 - u) - v;  a cross product's component is x.y y.z - x.z y.y etc.
#pragma once
#include "esr_common.h"

static_assert(sizeof(esr_bvh_node_t) == 64, "a node is 64 bytes");

// the mesh and its tree, as esr_bvh_cast takes them
struct BvhScene {
    const esr_bvh_node_t *nodes;
    int64_t n_f;
    const double *verts;
    int64_t n_v;
    const int64_t *tris;
};

struct Ray {
    double o[3], d[3], inv[3];
    double tmin;
};

struct Best {
    double t, u, v;
    int32_t face;
};

// The slab test of a box (binary32 corners) on [tmin, best], both ends included.  Conservative: every quotient is widened
// by the rounding it can carry, 2^-51 (|corner| + |o|) |1 / d|, so a box that holds a hit is never passed by.  An axis
// with d == 0 asks only whether o lies between the corners.  -> entered; `enter` is the entry distance
__device__ __forceinline__ bool slab(const Ray &r, const float *__restrict__ b, double best, double &enter)
{
#pragma clang fp contract(off)
    double lo = r.tmin, hi = best;
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double bl = (double)b[a], bh = (double)b[3 + a];
        ok = ok && bl <= bh;                                                  // (an empty box is never entered)
        if (r.d[a] == 0.0) {
            ok = ok && bl <= r.o[a] && r.o[a] <= bh;
            continue;
        }
        double t1, t2;
        if (fabs(r.inv[a]) < INFINITY) t1 = (bl - r.o[a]) * r.inv[a], t2 = (bh - r.o[a]) * r.inv[a];
        else t1 = (bl - r.o[a]) / r.d[a], t2 = (bh - r.o[a]) / r.d[a];
        const double err = (0x1p-51 * (fmax(fabs(bl), fabs(bh)) + fabs(r.o[a]))) * fabs(r.inv[a]);
        const double tn = fmin(t1, t2) - err, tf = fmax(t1, t2) + err;
        if (tn > lo) lo = tn;                                                  // (a NaN moves neither end)
        if (tf < hi) hi = tf;
    }
    enter = lo;
    return ok && lo <= hi;
}

__device__ __forceinline__ void triangle(const BvhScene &a, const Ray &r, int32_t f, int32_t skip, Best &best, double tmax)
{
#pragma clang fp contract(off)
    if (f == skip || (uint64_t)f >= (uint64_t)a.n_f) return;
    const int64_t id[3] = {a.tris[3 * (int64_t)f], a.tris[3 * (int64_t)f + 1], a.tris[3 * (int64_t)f + 2]};
    if ((uint64_t)id[0] >= (uint64_t)a.n_v || (uint64_t)id[1] >= (uint64_t)a.n_v || (uint64_t)id[2] >= (uint64_t)a.n_v) return;
    double p0[3], e1[3], e2[3], s[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        p0[i] = a.verts[3 * id[0] + i];
        e1[i] = a.verts[3 * id[1] + i] - p0[i];
        e2[i] = a.verts[3 * id[2] + i] - p0[i];
        s[i] = r.o[i] - p0[i];
    }
    const double px = r.d[1] * e2[2] - r.d[2] * e2[1];
    const double py = r.d[2] * e2[0] - r.d[0] * e2[2];
    const double pz = r.d[0] * e2[1] - r.d[1] * e2[0];
    const double det = (e1[0] * px + e1[1] * py) + e1[2] * pz;
    if (det == 0.0 || !(fabs(det) < INFINITY)) return;
    const double qx = s[1] * e1[2] - s[2] * e1[1];
    const double qy = s[2] * e1[0] - s[0] * e1[2];
    const double qz = s[0] * e1[1] - s[1] * e1[0];
    const double u = ((s[0] * px + s[1] * py) + s[2] * pz) / det;
    const double v = ((r.d[0] * qx + r.d[1] * qy) + r.d[2] * qz) / det;
    const double t = ((e2[0] * qx + e2[1] * qy) + e2[2] * qz) / det;
    const double w = (1.0 - u) - v;
    if (!(u >= 0.0 && v >= 0.0 && w >= 0.0 && t > r.tmin && t <= tmax)) return;
    if (t < best.t || (t == best.t && (best.face < 0 || f < best.face))) best.t = t, best.u = u, best.v = v, best.face = f;
}

// One ray against the scene: `best` comes in as {tmax, 0, 0, -1} and leaves with the nearest hit in (r.tmin, tmax] (ANY:
// with the first hit met).  `finite`: every component of o and d is; a ray that is not hits nothing.  n_box / n_tri count
// the boxes and triangles tested.  (A ray with a NaN end of its interval hits nothing: every comparison with it is false.)
template <bool ANY>
__device__ __forceinline__ void bvh_walk(const BvhScene &a, const Ray &r, bool finite, int32_t skip, double tmax, Best &best,
                                         int &n_box, int &n_tri)
{
    if (finite && a.n_f == 1) {
        triangle(a, r, 0, skip, best, tmax), ++n_tri;
    } else if (finite && a.n_f > 1) {
        uint64_t trail0 = 0, trail1 = 0;                                   // levels 0 .. 63 and 64 .. 127
        int32_t node = 0, came = -1;                                       // came: the side we return from, -1 entering
        int depth = 0;
        // (a tree is walked in under 3 steps a node; the bound only ends a walk over records that are no tree)
        for (uint32_t left = (uint32_t)min(8 * a.n_f, (int64_t)UINT32_MAX); left; --left) {
            const esr_bvh_node_t *nd = a.nodes + node;
            const int32_t child0 = nd->child[0], child1 = nd->child[1], parent = nd->parent;
            const uint64_t bit = (uint64_t)1 << (depth & 63);
            int first, stage;
            bool in0 = false, in1 = false;
            double enter0 = 0.0, enter1 = 0.0;
            if (came < 0) {
                in0 = slab(r, nd->box[0], best.t, enter0);
                in1 = slab(r, nd->box[1], best.t, enter1);
                n_box += 2;
                first = in1 && (!in0 || enter1 < enter0) ? 1 : 0;
                if (depth < 64) trail0 = (trail0 & ~bit) | (first ? bit : 0);
                else trail1 = (trail1 & ~bit) | (first ? bit : 0);
                stage = 0;
            } else {
                first = ((depth < 64 ? trail0 : trail1) & bit) ? 1 : 0;
                stage = came == first ? 1 : 2;
                if (stage == 1) {
                    double e;
                    const bool in = slab(r, first ? nd->box[0] : nd->box[1], best.t, e);
                    ++n_box;
                    if (first) in0 = in, enter0 = e;
                    else in1 = in, enter1 = e;
                }
            }
            int32_t down = -1;
            for (; stage < 2; ++stage) {
                const bool one = (stage == 0) == (first == 1);             // the side of this stage is child 1
                const bool in = one ? in1 : in0;
                const double e = one ? enter1 : enter0;
                const int32_t c = one ? child1 : child0;
                if (!in || !(e <= best.t)) continue;
                if (c >= 0) {
                    down = c;
                    break;
                }
                triangle(a, r, ~c, skip, best, tmax), ++n_tri;
                if (ANY && best.face >= 0) break;
            }
            if (ANY && best.face >= 0) break;
            if (down >= 0) {
                if ((int64_t)down >= a.n_f - 1 || depth >= 127) break;     // (a link outside the tree: never followed)
                node = down, came = -1, ++depth;
                continue;
            }
            if (parent < 0 || depth == 0) break;                           // back at the root: done
            node = parent >> 1, came = parent & 1, --depth;
            if ((int64_t)node >= a.n_f - 1) break;
        }
    }
}
