// Row f3 of SURVEY.md section 8: acceleration structures built ON THE DEVICE (cgrt_scene_set_build(CGRT_BUILD_DEVICE) or
// CGRT_BUILD=device).  Included by cgrt_hip.hip.  Two parts, both for OPAQUE owners (a transparent owner's improvement
// counter makes the reference's std::sort leaf order observable, quirk Q5: those keep the host build, cgrt_build.cpp):
//
//   (i)  bump floors -- Texture's height field (texture.h:28-35) and Plane's displacement mesh (objects.h:485-497) are
//        generated from the texture BYTES by two kernels: vertex heights, then one HCellRec (both triangles of a quad) per
//        cell in grid order plus the same TriRecs in construction order.  The device walks such a floor as a grid
//        (hfield_intersect), so no tree is needed at all.
//   (ii) opaque meshes -- the triangle-level hierarchy of tree_intersect_wide is built from the triangle soup: Morton
//        codes of the triangles' box centres, one radix sort (rocprim), a binary radix tree over the sorted codes
//        (Karras 2012: every inner node finds its own range and split, no recursion), boxes fitted bottom-up, groups of
//        <= 4 triangles as leaves, then the 4-wide form level by level with the host build's rule (replace the
//        larger-surfaced inner child by its children until there are four).  The walk's stack bound (kWideStack) is checked
//        on the device; a tree that misses it is rebuilt with balanced splits of the sorted order (depth <= log2 n).
//        build_mesh_core is that builder on a device vertex buffer, a stream and a scratch: the commit runs it with a temporary
//        scratch on the null stream, cgrt_scene_rebuild_mesh (cgrt_rebuild.hpp) with the handle's scratch on the caller's.
//
// Parity class: TOLERANCE, not bit-exact.  Boxes are supersets and the triangle test is the same
// code, so (len, triangle) of every ray with a UNIQUE nearest hit is bit-identical to the host build's.  What differs:
// exact ties (a ray through a shared edge or vertex) go to the triangle with the lower CONSTRUCTION index instead of the
// reference's leaf-order rule (objects.h:281,297) -- the two candidates share the hit point but not the normal --, and
// heights come from a correctly rounded exp (cgrt_ddexp.hpp) where the reference's libm is within 0.52 ulp.
#ifndef CGRT_DEVBUILD_HPP
#define CGRT_DEVBUILD_HPP
#include <rocprim/device/device_radix_sort.hpp>

#include "cgrt_ddexp.hpp"

namespace devbuild {

using namespace mesh_bounds;

// order-preserving map double -> uint64 (atomicMin / atomicMax on doubles of either sign)
__host__ __device__ inline unsigned long long dkey(double v) {
    union { double d; unsigned long long u; } c;
    c.d = v;
    return (c.u >> 63) ? ~c.u : (c.u | 0x8000000000000000ull);
}
__host__ __device__ inline double dunkey(unsigned long long k) {
    union { double d; unsigned long long u; } c;
    c.u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return c.d;
}
__device__ inline void atomic_min_max(unsigned long long *mm, double lo, double hi) {
    atomicMin(mm, dkey(lo));
    atomicMax(mm + 1, dkey(hi));
}
__device__ inline float f_down(double v) { return __double2float_rd(v); }  // largest float <= v (cgrt_build.cpp round_down)
__device__ inline float f_up(double v) { return __double2float_ru(v); }

// =====================================================================================================
// (i) bump floor
// =====================================================================================================
struct BumpArgs {
    const uint8_t *texels;  // rows x cols x 3
    int R, C;
    double p0, p2, lenx, leny, plane_y;
    int nx, nz;  // cells along x / z
    double *ys;  // (nz + 1) x (nx + 1) vertex heights (plane y included)
    unsigned long long *minmax;  // [0] = key of the lowest, [1] = of the highest vertex
    HCellRec *cells;
    HCellY *celly;
    TriRec *tris;
};

// texture.h:28-35 for the texels the mesh uses (every third row and column), objects.h:489-492: y = height + plane.y
__global__ void bump_vertex_kernel(BumpArgs a) {
    const int nv = (a.nx + 1) * (a.nz + 1);
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const int i = v / (a.nx + 1), j = v % (a.nx + 1);
    const uint8_t *q = a.texels + 3 * ((size_t)(i * 3) * a.C + (size_t)j * 3);
    const double luma = (0.299 * ((double)q[0] / 256.0) + 0.587 * ((double)q[1] / 256.0) + 0.114 * ((double)q[2] / 256.0));
    const double h = 1 - cgrt_dd::exp_dd(-3.3 * luma);
    const double y = h * 0.5 + a.plane_y;
    a.ys[v] = y;
    atomic_min_max(a.minmax, y, y);
}

// objects.h:485-497: quad (i, j) -> triangles (a, b, c) and (d, b, c), the host build's expressions term for term
__global__ void bump_cell_kernel(BumpArgs a) {
    const int nc = a.nx * a.nz;
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nc) return;
    const int i = c / a.nx, j = c % a.nx, step = 3;
    const double x1 = a.p0 + a.lenx * j * step / a.C;
    const double x2 = a.p0 + a.lenx * (j + 1) * step / a.C;
    const double z1 = a.p2 + a.leny * i * step / a.R;
    const double z2 = a.p2 + a.leny * (i + 1) * step / a.R;
    const int nxv = a.nx + 1;
    const double ya = a.ys[i * nxv + j], yb = a.ys[i * nxv + j + 1], yc = a.ys[(i + 1) * nxv + j], yd = a.ys[(i + 1) * nxv + j + 1];
    const double A[3] = {x1, ya, z1}, B[3] = {x2, yb, z1}, Cc[3] = {x1, yc, z2}, D[3] = {x2, yd, z2};
    HCellRec cell;
    cell.t[0] = make_tri_rec(A, B, Cc);
    cell.t[1] = make_tri_rec(D, B, Cc);
    // ties: no reference leaf order here -- the triangle with the lower construction index wins (header comment)
    cell.k[0] = 2 * c;
    cell.k[1] = 2 * c + 1;
    cell.leaf[0] = 0;
    cell.leaf[1] = 0;
    a.cells[c] = cell;
    HCellY cy;
    cy.lo = f_down(fmin(fmin(ya, yb), fmin(yc, yd)));
    cy.hi = f_up(fmax(fmax(ya, yb), fmax(yc, yd)));
    a.celly[c] = cy;
    a.tris[2 * c] = cell.t[0];
    a.tris[2 * c + 1] = cell.t[1];
}

// =====================================================================================================
// (ii) opaque mesh: LBVH -> groups of <= 4 -> 4-wide
// =====================================================================================================
struct MeshArgs {
    const double *tri9;  // n x 9
    int n;
    TriRec *tris;        // n, construction order
    OTriRec *otris;      // n, hierarchy order
    WideNodeRec *wnodes; // capacity n
    unsigned long long *gbox;  // 6 keys: min x,y,z then max x,y,z of all vertices (dkey), [6] = max squared vertex distance key
    unsigned long long *keys_in, *keys_out;
    unsigned int *idx_in, *idx_out;
    // binary tree: inner node i in [0, n-1), leaf j = n - 1 + j
    int *left, *right, *first, *last, *parent, *flag;
    double *box;  // (2n - 1) x 6: lo(3), hi(3)
    int2 *queue;  // wide-node work list: {binary node, stack entries waiting above it}
    int *tail;    // [0] = wide nodes so far, [1] = stack need, [2] = root (binary node id)
    int *range;   // wide_level_kernel's level: R_BEGIN, R_END (queue entries), R_LEVELS done so far, R_TICKET
};
enum { R_BEGIN = 0, R_END = 1, R_LEVELS = 2, R_TICKET = 3, N_RANGE = 4 };

// TriRec per triangle and the box of all vertices
__global__ void mesh_prep_kernel(MeshArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const double *t = a.tri9 + 9 * (size_t)i;
    a.tris[i] = make_tri_rec(t, t + 3, t + 6);
    double lo[3], hi[3];
    tri_box(t, lo, hi);
    for (int k = 0; k < 3; k++) {
        atomicMin(a.gbox + k, dkey(lo[k]));
        atomicMax(a.gbox + 3 + k, dkey(hi[k]));
    }
}

__device__ inline unsigned long long spread21(unsigned long long v) {  // 21 bits -> every third bit
    v &= 0x1fffffull;
    v = (v | (v << 32)) & 0x1f00000000ffffull;
    v = (v | (v << 16)) & 0x1f0000ff0000ffull;
    v = (v | (v << 8)) & 0x100f00f00f00f00full;
    v = (v | (v << 4)) & 0x10c30c30c30c30c3ull;
    v = (v | (v << 2)) & 0x1249249249249249ull;
    return v;
}

// Morton code of the triangle's box centre in the box of all vertices; also the largest squared vertex distance from that
// box's centre (the scene walk's bounding sphere, cgrt_build.cpp add_mesh_triangles)
__global__ void mesh_morton_kernel(MeshArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    double glo[3], ghi[3];
    for (int k = 0; k < 3; k++) {
        glo[k] = dunkey(a.gbox[k]);
        ghi[k] = dunkey(a.gbox[3 + k]);
    }
    const double *t = a.tri9 + 9 * (size_t)i;
    double lo[3], hi[3];
    tri_box(t, lo, hi);
    unsigned long long code = 0;
    for (int k = 0; k < 3; k++) {
        const double ext = ghi[k] - glo[k];
        double q = ext > 0 ? (0.5 * (lo[k] + hi[k]) - glo[k]) / ext * 2097152.0 : 0.0;
        q = q < 0 ? 0 : (q > 2097151.0 ? 2097151.0 : q);
        code |= spread21((unsigned long long)q) << k;
    }
    a.keys_in[i] = code;
    a.idx_in[i] = (unsigned int)i;
    const double c[3] = {0.5 * (glo[0] + ghi[0]), 0.5 * (glo[1] + ghi[1]), 0.5 * (glo[2] + ghi[2])};
    double r2 = 0;
    for (int v = 0; v < 3; v++) r2 = fmax(r2, dist2(t + 3 * v, c));
    atomicMax(a.gbox + 6, dkey(r2));
}

// length of the common prefix of sorted keys i and j (equal keys: continued on the index bits); -1 outside the array
__device__ inline int lcp(const unsigned long long *keys, int n, int i, int j) {
    if (j < 0 || j >= n) return -1;
    const unsigned long long x = keys[i] ^ keys[j];
    return x ? __clzll((long long)x) : 64 + __clz(i ^ j);
}

// Karras 2012, "Maximizing parallelism in the construction of BVHs, octrees and k-d trees", section 4: inner node i
__global__ void lbvh_nodes_kernel(MeshArgs a) {
    const int n = a.n;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n - 1) return;
    const unsigned long long *keys = a.keys_out;
    const int d = (lcp(keys, n, i, i + 1) - lcp(keys, n, i, i - 1)) >= 0 ? 1 : -1;
    const int dmin = lcp(keys, n, i, i - d);
    int lmax = 2;
    while (lcp(keys, n, i, i + lmax * d) > dmin) lmax *= 2;
    int l = 0;
    for (int t = lmax / 2; t >= 1; t /= 2)
        if (lcp(keys, n, i, i + (l + t) * d) > dmin) l += t;
    const int j = i + l * d;
    const int dnode = lcp(keys, n, i, j);
    int s = 0, t = l;
    do {
        t = (t + 1) / 2;
        if (lcp(keys, n, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int gamma = i + s * d + (d < 0 ? d : 0);
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    const int L = (lo == gamma) ? n - 1 + gamma : gamma;
    const int Rr = (hi == gamma + 1) ? n - 1 + gamma + 1 : gamma + 1;
    a.left[i] = L;
    a.right[i] = Rr;
    a.first[i] = lo;
    a.last[i] = hi;
    a.parent[L] = i;
    a.parent[Rr] = i;
    if (i == 0) {
        a.parent[0] = -1;
        a.tail[2] = 0;
    }
}

// The fallback: balanced splits of the sorted order -- the inner node that splits between sorted triangles s and s + 1 is
// node s; its range is found by descending from the root (<= log2 n steps)
__global__ void balanced_nodes_kernel(MeshArgs a) {
    const int n = a.n;
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n - 1) return;
    int b = 0, e = n - 1, par = -1, mid;
    while (true) {
        mid = (b + e) / 2;
        if (mid == s) break;
        par = mid;
        if (s < mid) e = mid;
        else b = mid + 1;
    }
    const int L = (b == mid) ? n - 1 + b : (b + mid) / 2;
    const int Rr = (mid + 1 == e) ? n - 1 + e : (mid + 1 + e) / 2;
    a.left[s] = L;
    a.right[s] = Rr;
    a.first[s] = b;
    a.last[s] = e;
    a.parent[s] = par;
    if (L >= n - 1) a.parent[L] = s;
    if (Rr >= n - 1) a.parent[Rr] = s;
    if (par < 0) a.tail[2] = s;
}

// boxes bottom-up: one thread per sorted triangle; the second thread to reach an inner node fits it and goes on
__global__ void lbvh_fit_kernel(MeshArgs a) {
    const int n = a.n;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const unsigned int src = a.idx_out[j];
    const double *t = a.tri9 + 9 * (size_t)src;
    double lo[3], hi[3];
    tri_box(t, lo, hi);
    double *bx = a.box + 6 * (size_t)(n - 1 + j);
    for (int k = 0; k < 3; k++) {
        bx[k] = lo[k];
        bx[3 + k] = hi[k];
    }
    // the hierarchy's own triangle order: record + construction index (ties: lower index wins, see the header comment)
    OTriRec o;
    o.t = a.tris[src];
    o.k = (int32_t)src;
    o.leaf = 0;
    a.otris[j] = o;
    if (n == 1) {
        a.tail[2] = 0;  // the root is leaf 0 (id n - 1 + 0 = 0)
        return;
    }
    int node = a.parent[n - 1 + j];
    while (node >= 0) {
        __threadfence();
        if (atomicAdd(&a.flag[node], 1) == 0) return;  // the sibling subtree is not fitted yet: its thread will come by
        __threadfence();
        const volatile double *lb = a.box + 6 * (size_t)a.left[node], *rb = a.box + 6 * (size_t)a.right[node];
        double *nb = a.box + 6 * (size_t)node;
        for (int k = 0; k < 3; k++) {
            nb[k] = fmin(lb[k], rb[k]);
            nb[3 + k] = fmax(lb[3 + k], rb[3 + k]);
        }
        node = a.parent[node];
    }
}

__device__ inline bool group_leaf(const MeshArgs &a, int node, int &first, int &cnt) {
    const int n = a.n;
    if (node >= n - 1) {
        first = node - (n - 1);
        cnt = 1;
        return true;
    }
    first = a.first[node];
    cnt = a.last[node] - first + 1;
    return cnt <= 4;  // HostTree::build_bvh: max_leaf = 4
}

// mesh_prep_kernel's starting values, written on the stream (no upload): the keys of an empty box and of radius 0
__global__ void mesh_init_kernel(MeshArgs a) {
    if (blockIdx.x != 0 || threadIdx.x >= 7) return;
    a.gbox[threadIdx.x] = threadIdx.x < 3 ? ~0ull : 0ull;
}

// The wide form's starting state, once the binary tree's root is known (tail[2]): queue[0] = the root, one wide node so far,
// level [0, 1), no ticket taken
__global__ void wide_init_kernel(MeshArgs a) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    a.queue[0] = make_int2(a.tail[2], 0);
    a.tail[0] = 1;
    a.tail[1] = 0;
    a.range[R_BEGIN] = 0;
    a.range[R_END] = 1;
    a.range[R_LEVELS] = 0;
    a.range[R_TICKET] = 0;
}

// One level of the 4-wide form (BvhBuilder::emit_wide's rule): queue entries [begin, end) become wnodes[begin, end); their
// inner children are appended to the queue for the next launch.  The level's range is read from device memory
// (range[R_BEGIN], range[R_END]) and walked grid-stride, so the host enqueues launch after launch without reading anything
// back: the last workgroup of a launch to finish -- told by the value its agent-scope add to range[R_TICKET] returns -- rotates
// the range for the NEXT launch (begin = end, end = tail[0]).  Every add to tail[0] of the launch has returned before its
// workgroup takes a ticket, and all of them are agent-scope atomics on one word, so the last ticket's atomic load of tail[0]
// sees the level's final count.  No workgroup waits for another (refit_nodes_kernel's rule); the range words are written by
// one workgroup after every other has read them, and are read again only by the next launch.  A launch on an empty level
// returns at once, without a ticket (all its workgroups see the same empty range).
__global__ __launch_bounds__(256) void wide_level_kernel(MeshArgs a) {
    const int begin = a.range[R_BEGIN], end = a.range[R_END] < a.n ? a.range[R_END] : a.n;  // (queue and wnodes hold n)
    if (begin >= end) return;
    int need = 0;
    for (int q = begin + (int)(blockIdx.x * blockDim.x + threadIdx.x); q < end; q += (int)(gridDim.x * blockDim.x)) {
        const int node = a.queue[q].x, acc = a.queue[q].y;
        int kids[4], nk = 0, f, c;
        if (group_leaf(a, node, f, c)) {
            kids[nk++] = node;  // a tree that is one leaf: a root with that one child
        } else {
            kids[nk++] = a.left[node];
            kids[nk++] = a.right[node];
            while (nk < 4) {
                int best = -1;
                double best_area = -1;
                for (int k = 0; k < nk; k++) {
                    if (group_leaf(a, kids[k], f, c)) continue;
                    const double *b = a.box + 6 * (size_t)kids[k];
                    const double x = b[3] - b[0], y = b[4] - b[1], z = b[5] - b[2];
                    const double area = x * y + y * z + z * x;
                    if (area > best_area) {
                        best_area = area;
                        best = k;
                    }
                }
                if (best < 0) break;
                const int cnode = kids[best];
                kids[best] = a.left[cnode];
                kids[nk++] = a.right[cnode];
            }
        }
        WideNodeRec w;
        for (int k = 0; k < 4; k++) {
            w.pad[k] = 0;
            if (k >= nk) {
                w.lox[k] = w.loy[k] = w.loz[k] = w.hix[k] = w.hiy[k] = w.hiz[k] = 0.f;
                w.ref[k] = kWideNone;
                continue;
            }
            const double *b = a.box + 6 * (size_t)kids[k];
            w.lox[k] = f_down(b[0] - kBoxPad);
            w.loy[k] = f_down(b[1] - kBoxPad);
            w.loz[k] = f_down(b[2] - kBoxPad);
            w.hix[k] = f_up(b[3] + kBoxPad);
            w.hiy[k] = f_up(b[4] + kBoxPad);
            w.hiz[k] = f_up(b[5] + kBoxPad);
            if (group_leaf(a, kids[k], f, c)) {
                w.ref[k] = (int32_t)(((uint32_t)f << 4) | (uint32_t)c);
            } else {
                const int child = atomicAdd(&a.tail[0], 1);
                if (child < a.n) a.queue[child] = make_int2(kids[k], acc + nk - 1);  // (never more nodes than triangles: the host checks)
                w.ref[k] = ~child;
            }
        }
        need = need > acc + nk - 1 ? need : acc + nk - 1;
        a.wnodes[q] = w;
    }
    if (need > 0) atomicMax(&a.tail[1], need);
    // every atomic of this workgroup has been performed before its ticket is taken
    __threadfence();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int ticket = __hip_atomic_fetch_add(&a.range[R_TICKET], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (ticket != (int)gridDim.x - 1) return;
    const int total = __hip_atomic_load(&a.tail[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&a.range[R_BEGIN], end, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&a.range[R_END], total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&a.range[R_LEVELS], a.range[R_LEVELS] + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&a.range[R_TICKET], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Cover spheres for classify_kernel (cgrt_build.cpp cover_spheres): group g = sorted triangles [g n / G, (g + 1) n / G) --
// contiguous in Morton order, hence compact --, sphere = (centre of the group's vertex box, largest vertex distance + 1e-3).
// One workgroup per group (no group is empty: cover_groups leaves 64 triangles or more to each, or all to the one).
__global__ __launch_bounds__(kReduceThreads) void cover_kernel(MeshArgs a, int G, double *cover) {
    __shared__ double part[4 * 6];
    const int g = blockIdx.x, n = a.n;
    const int b = (int)((long long)g * n / G), e = (int)((long long)(g + 1) * n / G);
    double c[3], r2[2];
    range_sphere(a.tri9, reinterpret_cast<const int *>(a.idx_out), 1, b, e, nullptr, part, c, r2);
    if (threadIdx.x == 0) store_cover(cover + 4 * (size_t)g, c, r2[0], true, c);
}

// ---- host drivers --------------------------------------------------------------------------------------------------

struct BumpResult {
    double ylo = 0, yhi = 0;
};
// texels: device pointer to this texture's bytes; cells / tris: where the records go (device)
static int build_bump_floor(const uint8_t *texels, int R, int C, const double p[3], double lenx, double leny, double plane_y,
                            HCellRec *cells, HCellY *celly, TriRec *tris, BumpResult &out) {
    BumpArgs a;
    a.texels = texels;
    a.R = R;
    a.C = C;
    a.p0 = p[0];
    a.p2 = p[2];
    a.lenx = lenx;
    a.leny = leny;
    a.plane_y = plane_y;
    a.nx = C / 3 - 1;
    a.nz = R / 3 - 1;
    a.cells = cells;
    a.celly = celly;
    a.tris = tris;
    const int nv = (a.nx + 1) * (a.nz + 1), nc = a.nx * a.nz;
    DevBuf ys, mm;
    HIP_TRY(ys.alloc((size_t)nv * sizeof(double)));
    HIP_TRY(mm.alloc(2 * sizeof(unsigned long long)));
    const unsigned long long init[2] = {~0ull, 0ull};
    HIP_TRY(hipMemcpy(mm.p, init, sizeof(init), hipMemcpyHostToDevice));
    a.ys = ys.as<double>();
    a.minmax = mm.as<unsigned long long>();
    hipLaunchKernelGGL(bump_vertex_kernel, dim3((nv + 255) / 256), dim3(256), 0, 0, a);
    hipLaunchKernelGGL(bump_cell_kernel, dim3((nc + 255) / 256), dim3(256), 0, 0, a);
    HIP_TRY(hipGetLastError());
    unsigned long long got[2];
    HIP_TRY(hipMemcpy(got, mm.p, sizeof(got), hipMemcpyDeviceToHost));  // synchronises
    out.ylo = dunkey(got[0]);
    out.yhi = dunkey(got[1]);
    return CGRT_OK;
}

struct MeshResult {
    int nwide = 0, stack_need = 0;
    bool balanced = false;  // the fallback build was needed
    int levels = 0, readbacks = 0;  // of the 4-wide form; of its level counters (one per batch of levels)
    double centre[3] = {0, 0, 0}, r2 = -1.0;  // ObjRec.a / s0 (bounding sphere of the vertices, grown like the host's)
    float bmax = 0;  // TreeRec::bmax (tree_bmax of the largest |coordinate| of a vertex)
    std::vector<double> cover;  // n_groups x (cx, cy, cz, r)
};

// cover spheres of a mesh of n triangles: a function of n alone
static inline int cover_groups(int n) {
    int depth = 0;
    while (depth < 6 && (n >> (depth + 1)) >= 64) depth++;
    return 1 << depth;
}

// Everything a build of n triangles needs besides its input and its three destinations, in ONE allocation: the commit makes a
// temporary one per mesh (with room for the uploaded vertices), a rebuild keeps one on the handle (with staging records)
struct MeshScratch {
    DevBuf mem;
    size_t bytes = 0, sort_bytes = 0;
    int n = 0, G = 0;
    unsigned long long *gbox = nullptr, *keys_in = nullptr, *keys_out = nullptr;
    unsigned int *idx_in = nullptr, *idx_out = nullptr;
    int *tree = nullptr, *tail = nullptr;  // tail[4] then range[N_RANGE]: one read-back
    double *box = nullptr, *cover = nullptr, *tri9 = nullptr;
    int2 *queue = nullptr;
    void *sort_tmp = nullptr;
    TriRec *tris = nullptr;  // staging (rebuild only)
    OTriRec *otris = nullptr;
    WideNodeRec *wnodes = nullptr;

    int alloc(int n_, bool with_tri9, bool with_staging) {
        n = n_;
        G = cover_groups(n);
        const size_t N = (size_t)n;
        HIP_TRY(rocprim::radix_sort_pairs(nullptr, sort_bytes, keys_in, keys_out, idx_in, idx_out, N, 0u, 63u, (hipStream_t)0));  // (sizes only)
        size_t at = 0;
        auto take = [&at](size_t b) { const size_t o = at; at += (b + 255) & ~(size_t)255; return o; };
        const size_t o_gbox = take(8 * sizeof(unsigned long long)), o_tail = take((4 + N_RANGE) * sizeof(int));
        const size_t o_k0 = take(N * 8), o_k1 = take(N * 8), o_i0 = take(N * 4), o_i1 = take(N * 4);
        const size_t o_tree = take(7 * N * sizeof(int));  // left, right, first, last, flag: n - 1 each; parent: 2n - 1
        const size_t o_box = take(2 * N * 6 * sizeof(double)), o_queue = take(N * sizeof(int2));
        const size_t o_cover = take((size_t)G * 4 * sizeof(double)), o_sort = take(sort_bytes);
        const size_t o_tri9 = take(with_tri9 ? N * 9 * sizeof(double) : 0);
        const size_t o_tris = take(with_staging ? N * sizeof(TriRec) : 0), o_otris = take(with_staging ? N * sizeof(OTriRec) : 0);
        const size_t o_wnodes = take(with_staging ? N * sizeof(WideNodeRec) : 0);
        HIP_TRY(mem.alloc(at));
        bytes = at;
        unsigned char *m = mem.as<unsigned char>();
        gbox = reinterpret_cast<unsigned long long *>(m + o_gbox);
        tail = reinterpret_cast<int *>(m + o_tail);
        keys_in = reinterpret_cast<unsigned long long *>(m + o_k0);
        keys_out = reinterpret_cast<unsigned long long *>(m + o_k1);
        idx_in = reinterpret_cast<unsigned int *>(m + o_i0);
        idx_out = reinterpret_cast<unsigned int *>(m + o_i1);
        tree = reinterpret_cast<int *>(m + o_tree);
        box = reinterpret_cast<double *>(m + o_box);
        queue = reinterpret_cast<int2 *>(m + o_queue);
        cover = reinterpret_cast<double *>(m + o_cover);
        sort_tmp = m + o_sort;
        tri9 = with_tri9 ? reinterpret_cast<double *>(m + o_tri9) : nullptr;
        tris = with_staging ? reinterpret_cast<TriRec *>(m + o_tris) : nullptr;
        otris = with_staging ? reinterpret_cast<OTriRec *>(m + o_otris) : nullptr;
        wnodes = with_staging ? reinterpret_cast<WideNodeRec *>(m + o_wnodes) : nullptr;
        return CGRT_OK;
    }
};

static int env_int(const char *name, int lo, int hi, int dflt) {
    const char *e = std::getenv(name);
    if (!e || !*e) return dflt;
    const long v = std::strtol(e, nullptr, 10);
    return v < lo ? lo : (v > hi ? hi : (int)v);
}

// The builder: tri9 (DEVICE, n x 9 doubles) -> tris / otris / wnodes (device destinations of n records each) and out, with every
// launch and copy on stream st, which it synchronises: once per batch of levels for the level counters, once at the end for the
// bounds.  Nothing is allocated here and no initial value is uploaded.
static int build_mesh_core(const double *tri9, int n, hipStream_t st, MeshScratch &S, TriRec *tris, OTriRec *otris,
                           WideNodeRec *wnodes, MeshResult &out) {
    out = MeshResult();
    if (n <= 0) return CGRT_OK;
    const size_t N = (size_t)n;
    MeshArgs a;
    a.tri9 = tri9;
    a.n = n;
    a.tris = tris;
    a.otris = otris;
    a.wnodes = wnodes;
    a.gbox = S.gbox;
    a.keys_in = S.keys_in;
    a.keys_out = S.keys_out;
    a.idx_in = S.idx_in;
    a.idx_out = S.idx_out;
    int *tp = S.tree;
    a.left = tp;
    a.right = tp + N;
    a.first = tp + 2 * N;
    a.last = tp + 3 * N;
    a.flag = tp + 4 * N;
    a.parent = tp + 5 * N;
    a.box = S.box;
    a.queue = S.queue;
    a.tail = S.tail;
    a.range = S.tail + 4;
    const dim3 blk(256), grd((unsigned)((N + 255) / 256));
    hipLaunchKernelGGL(mesh_init_kernel, dim3(1), dim3(64), 0, st, a);
    hipLaunchKernelGGL(mesh_prep_kernel, grd, blk, 0, st, a);
    hipLaunchKernelGGL(mesh_morton_kernel, grd, blk, 0, st, a);
    size_t tmp_bytes = S.sort_bytes;
    HIP_TRY(rocprim::radix_sort_pairs(S.sort_tmp, tmp_bytes, a.keys_in, a.keys_out, a.idx_in, a.idx_out, N, 0u, 63u, st));
    // Test aids, read at every build.  CGRT_DEVBUILD_BALANCED=1: skip the radix tree and take the fallback at once;
    // CGRT_REBUILD_BATCH: levels enqueued per read-back; CGRT_REBUILD_GRID: workgroups of a level's launch
    int first_attempt = 0;
    if (const char *e = std::getenv("CGRT_DEVBUILD_BALANCED")) first_attempt = (*e && *e != '0') ? 1 : 0;
    const int batch = env_int("CGRT_REBUILD_BATCH", 1, 64, 8);
    const int grid = env_int("CGRT_REBUILD_GRID", 1, 1024, (int)std::min<size_t>(256, (N + 1023) / 1024));
    for (int attempt = first_attempt; attempt < 2; attempt++) {
        HIP_TRY(hipMemsetAsync(a.flag, 0, N * sizeof(int), st));
        if (n > 1) {
            if (attempt == 0) hipLaunchKernelGGL(lbvh_nodes_kernel, grd, blk, 0, st, a);
            else hipLaunchKernelGGL(balanced_nodes_kernel, grd, blk, 0, st, a);
        }
        hipLaunchKernelGGL(lbvh_fit_kernel, grd, blk, 0, st, a);
        // the wide form, level by level, a batch of levels per read-back of {nwide, stack need, root | begin, end, levels, ticket}
        hipLaunchKernelGGL(wide_init_kernel, dim3(1), dim3(64), 0, st, a);
        int t[4 + N_RANGE];
        for (int rounds = 0;; rounds++) {
            for (int b = 0; b < batch; b++) hipLaunchKernelGGL(wide_level_kernel, dim3((unsigned)grid), blk, 0, st, a);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(t, S.tail, sizeof(t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            out.readbacks++;
            if (t[0] > n) return fail(CGRT_ERR_DEVICE, "device hierarchy build: more wide nodes than triangles");
            if (t[4 + R_BEGIN] >= t[4 + R_END]) break;
            if ((long long)rounds * batch > (long long)n + 1) return fail(CGRT_ERR_DEVICE, "device hierarchy build: more levels than triangles");
        }
        out.nwide = t[0];
        out.stack_need = t[1];
        out.levels = t[4 + R_LEVELS];
        out.balanced = attempt == 1;
        if (out.stack_need < kWideStack) break;
        if (attempt == 1) return fail(CGRT_ERR_LIMIT, "device hierarchy build: stack bound missed by the balanced tree");
    }
    // bounding sphere (add_mesh_triangles) and cover spheres (cover_spheres)
    hipLaunchKernelGGL(cover_kernel, dim3((unsigned)S.G), dim3(kReduceThreads), 0, st, a, S.G, S.cover);
    HIP_TRY(hipGetLastError());
    unsigned long long g[7];
    out.cover.resize((size_t)S.G * 4);
    HIP_TRY(hipMemcpyAsync(g, S.gbox, sizeof(g), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out.cover.data(), S.cover, out.cover.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    double max_abs = 0;
    for (int k = 0; k < 3; k++) {
        out.centre[k] = 0.5 * (dunkey(g[k]) + dunkey(g[3 + k]));
        max_abs = std::max(max_abs, std::max(std::fabs(dunkey(g[k])), std::fabs(dunkey(g[3 + k]))));
    }
    out.bmax = tree_bmax(max_abs);
    out.r2 = sphere_s0(cover_radius(dunkey(g[6])));
    return CGRT_OK;
}

// The commit's form: tri9_host: n x 9 doubles; tris / otris / wnodes: device destinations (n, n, n records).  A temporary
// scratch, the null stream.
static int build_mesh_hierarchy(const double *tri9_host, int n, TriRec *tris, OTriRec *otris, WideNodeRec *wnodes, MeshResult &out) {
    out = MeshResult();
    if (n <= 0) return CGRT_OK;
    MeshScratch S;
    if (const int rc = S.alloc(n, true, false)) return rc;
    HIP_TRY(hipMemcpy(S.tri9, tri9_host, (size_t)n * 9 * sizeof(double), hipMemcpyHostToDevice));
    return build_mesh_core(S.tri9, n, (hipStream_t)0, S, tris, otris, wnodes, out);
}

}  // namespace devbuild
#endif
