// Wave-packet ray tracing through the evolving flow (include/sw.h sw_rays_*,
// DESIGN.md §9): the packets of raytracing/GPURaytracing.jl:22-65 kept on
// the device next to the flow state.
//
//   ω = sign √(f² + Cg²(k² + l²))
//   ẋ = U + Cg² k/ω        k̇ = -(U_x k + V_x l)
//   ẏ = V + Cg² l/ω        l̇ = -(U_y k + V_y l),  V_y = -U_x
//
// U … V_x are sampled with periodic bilinear weights from "texel" snapshots:
// one 64-byte record {u, v, u_x, u_y, v_x, 0, 0, 0} per grid point, x fastest,
// nodes at x_i = -Lx/2 + i dx, y_j = -Ly/2 + j dy.  A right-hand side needs
// 5 fields × 4 corners × 2 snapshots: from records that is one 40-byte read
// per corner and snapshot (the two x-neighbours contiguous) instead of 40
// scattered 8-byte reads from ten planes.
//
// Work split: four lanes per packet, one per bilinear corner.  Each lane
// gathers its corner's record from the old and the new snapshot, blends and
// weights it; the quad is summed with two DPP quad permutes (no LDS) in the
// fixed order (c00 + c10) + (c01 + c11), after which every lane of the quad
// holds the five sums and advances its own copy of the packet.  All nsub RK4
// substeps run in one launch with the packet in registers; lane 0 stores.
#include "sw_internal.hpp"

namespace sw {
namespace {

constexpr int RAY_BLOCK = 256;
// lanes per packet: 4 (the quad split), or 1 with -DSW_RAYS_PER_THREAD (the
// comparison build of tools/rays_cadence.py --ab: every thread walks the four
// corners itself, same sums in the same order)
#ifdef SW_RAYS_PER_THREAD
constexpr int RAY_LANES = 1;
#else
constexpr int RAY_LANES = 4;
#endif

struct Fields {
  double u, v, ux, uy, vx;
};
struct Packet {
  double x, y, k, l;
};

// the value of lane (lane ^ 1) / (lane ^ 2) of this quad: v_mov_b32 with
// quad_perm [1,0,3,2] (0xB1) / [2,3,0,1] (0x4E) on each half.  Every lane of
// the block is active where this is called (no early exits in the kernels).
template <int CTRL>
__device__ __forceinline__ double quad_peer(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double quad_sum(double v) {
  v = v + quad_peer<0xB1>(v);  // lanes 0,1: c00 + c10; lanes 2,3: c01 + c11
  v = v + quad_peer<0x4E>(v);  // (c00 + c10) + (c01 + c11), commuted on lanes 2,3
  return v;
}

// Cell of coordinate x on a periodic axis of n nodes: i0 and its right
// neighbour i1 (wrapped), fr the weight of i1.  The indices are in [0, n) for
// every bit pattern of x: the position is reduced in floating point first, and
// a NaN or Inf (a flow that blew up) fails both comparisons -> i0 = 0, while
// fr stays NaN: it reaches the values, never an address.
__device__ __forceinline__ void ray_cell(double x, double x0, double rd, int n, int& i0, int& i1, double& fr) {
  const double dn = (double)n;
  double s = (x - x0) * rd;
  s -= dn * floor(s / dn);
  if (s >= dn) s = 0.0;  // s = -tiny rounds to n: node 0
  i0 = (s >= 0.0 && s < dn) ? (int)s : 0;
  i1 = i0 + 1 == n ? 0 : i0 + 1;
  fr = s - (double)i0;
}

// w × the blended record of node (i, j): three 16-byte loads per snapshot
template <bool BLEND>
__device__ __forceinline__ Fields ray_corner(const RayGrid& rg, const double2* __restrict__ texo,
                                             const double2* __restrict__ texn, int i, int j, double w, double a) {
  const long long o = ((long long)j * rg.nx + i) * RAY_TEXEL;
  const double2 n0 = texn[o], n1 = texn[o + 1], n2 = texn[o + 2];
  Fields r{n0.x, n0.y, n1.x, n1.y, n2.x};
  if (BLEND) {
    const double2 o0 = texo[o], o1 = texo[o + 1], o2 = texo[o + 2];
    const double b = 1.0 - a;
    r.u = b * o0.x + a * r.u;
    r.v = b * o0.y + a * r.v;
    r.ux = b * o1.x + a * r.ux;
    r.uy = b * o1.y + a * r.uy;
    r.vx = b * o2.x + a * r.vx;
  }
  return Fields{w * r.u, w * r.v, w * r.ux, w * r.uy, w * r.vx};
}

// the five fields at (x, y), time fraction a; c = this lane's corner (x bit 0, y bit 1)
template <bool BLEND>
__device__ __forceinline__ Fields ray_gather(const RayGrid& rg, const double2* __restrict__ texo,
                                             const double2* __restrict__ texn, double x, double y, double a,
                                             int c) {
  int i0, i1, j0, j1;
  double fx, fy;
  ray_cell(x, rg.x0, rg.rdx, rg.nx, i0, i1, fx);
  ray_cell(y, rg.y0, rg.rdy, rg.ny, j0, j1, fy);
  const double gx = 1.0 - fx, gy = 1.0 - fy;
  if (RAY_LANES == 4) {
    const bool cx = c & 1, cy = c & 2;
    const Fields t = ray_corner<BLEND>(rg, texo, texn, cx ? i1 : i0, cy ? j1 : j0, (cx ? fx : gx) * (cy ? fy : gy), a);
    return Fields{quad_sum(t.u), quad_sum(t.v), quad_sum(t.ux), quad_sum(t.uy), quad_sum(t.vx)};
  }
  const Fields a00 = ray_corner<BLEND>(rg, texo, texn, i0, j0, gx * gy, a);
  const Fields a10 = ray_corner<BLEND>(rg, texo, texn, i1, j0, fx * gy, a);
  const Fields a01 = ray_corner<BLEND>(rg, texo, texn, i0, j1, gx * fy, a);
  const Fields a11 = ray_corner<BLEND>(rg, texo, texn, i1, j1, fx * fy, a);
  return Fields{(a00.u + a10.u) + (a01.u + a11.u), (a00.v + a10.v) + (a01.v + a11.v),
                (a00.ux + a10.ux) + (a01.ux + a11.ux), (a00.uy + a10.uy) + (a01.uy + a11.uy),
                (a00.vx + a10.vx) + (a01.vx + a11.vx)};
}

// dxkdt (raytracing/GPURaytracing.jl:32-65) at one packet
template <bool BLEND>
__device__ __forceinline__ Packet ray_rhs(const RayGrid& rg, const RayPhys& rp, const double2* __restrict__ texo,
                                          const double2* __restrict__ texn, const Packet& s, double sg, double a,
                                          int c) {
  const Fields F = ray_gather<BLEND>(rg, texo, texn, s.x, s.y, a, c);
  const double om = sg * sqrt(rp.f * rp.f + rp.Cg2 * (s.k * s.k + s.l * s.l));
  return Packet{F.u + rp.Cg2 * s.k / om, F.v + rp.Cg2 * s.l / om, -(F.ux * s.k + F.vx * s.l),
                -(F.uy * s.k - F.ux * s.l)};
}
__device__ __forceinline__ Packet ray_axpy(const Packet& s, double h, const Packet& d) {
  return Packet{s.x + h * d.x, s.y + h * d.y, s.k + h * d.k, s.l + h * d.l};
}

// packet and corner of this thread; threads past the last packet recompute
// packet n - 1 (and store nothing), so every lane of every quad stays active
__device__ __forceinline__ long long ray_thread(long long n, int& c, bool& store) {
  const long long gid = (long long)blockIdx.x * RAY_BLOCK + threadIdx.x;
  const long long q = gid / RAY_LANES;
  c = (int)(gid % RAY_LANES);
  store = q < n && c == 0;
  return q < n ? q : n - 1;
}

template <bool BLEND>
__global__ void __launch_bounds__(RAY_BLOCK)
    k_rays_trace(RayGrid rg, RayPhys rp, const double2* __restrict__ texo, const double2* __restrict__ texn,
                 double* __restrict__ xk, const double* __restrict__ sign, long long n, double h, int nsub) {
  int c;
  bool store;
  const long long p = ray_thread(n, c, store);
  Packet s{xk[p], xk[n + p], xk[2 * n + p], xk[3 * n + p]};
  const double sg = sign[p];
  for (int m = 0; m < nsub; ++m) {  // classical RK4, the blend at the stage times
    const double a0 = (double)m / (double)nsub, am = ((double)m + 0.5) / (double)nsub,
                 a1 = ((double)m + 1.0) / (double)nsub;
    const Packet k1 = ray_rhs<BLEND>(rg, rp, texo, texn, s, sg, a0, c);
    const Packet k2 = ray_rhs<BLEND>(rg, rp, texo, texn, ray_axpy(s, 0.5 * h, k1), sg, am, c);
    const Packet k3 = ray_rhs<BLEND>(rg, rp, texo, texn, ray_axpy(s, 0.5 * h, k2), sg, am, c);
    const Packet k4 = ray_rhs<BLEND>(rg, rp, texo, texn, ray_axpy(s, h, k3), sg, a1, c);
    const double w = h / 6.0;
    s.x = s.x + w * ((k1.x + 2.0 * k2.x) + (2.0 * k3.x + k4.x));
    s.y = s.y + w * ((k1.y + 2.0 * k2.y) + (2.0 * k3.y + k4.y));
    s.k = s.k + w * ((k1.k + 2.0 * k2.k) + (2.0 * k3.k + k4.k));
    s.l = s.l + w * ((k1.l + 2.0 * k2.l) + (2.0 * k3.l + k4.l));
  }
  if (store) {
    xk[p] = s.x;
    xk[n + p] = s.y;
    xk[2 * n + p] = s.k;
    xk[3 * n + p] = s.l;
  }
}

// savepacketdata! (raytracing/RaytracingDriver.jl:110-124): one snapshot at the packets
__global__ void __launch_bounds__(RAY_BLOCK)
    k_rays_sample(RayGrid rg, const double2* __restrict__ tex, const double* __restrict__ xk, long long n,
                  double* __restrict__ U, double* __restrict__ G) {
  int c;
  bool store;
  const long long p = ray_thread(n, c, store);
  const Fields F = ray_gather<false>(rg, nullptr, tex, xk[p], xk[n + p], 1.0, c);
  if (store) {
    U[p] = F.u;
    U[n + p] = F.v;
    G[p] = F.ux;
    G[n + p] = F.uy;
    G[2 * n + p] = F.vx;
    G[3 * n + p] = -F.ux;
  }
}

// five planes -> texels: a thread reads its point of each plane (coalesced)
// and writes its record with four 16-byte stores, a wave 4 KB contiguously
__global__ void __launch_bounds__(RAY_BLOCK)
    k_rays_pack(long long np, const double* __restrict__ planes, double2* __restrict__ tex) {
  const long long i = (long long)blockIdx.x * RAY_BLOCK + threadIdx.x;
  if (i >= np) return;
  double2* t = tex + i * RAY_TEXEL;
  t[0] = make_double2(planes[i], planes[np + i]);
  t[1] = make_double2(planes[2 * np + i], planes[3 * np + i]);
  t[2] = make_double2(planes[4 * np + i], 0.0);
  t[3] = make_double2(0.0, 0.0);
}

inline dim3 ray_grid(long long n) { return dim3((unsigned)((n * RAY_LANES + RAY_BLOCK - 1) / RAY_BLOCK)); }

}  // namespace

void launch_rays_pack(const RayGrid& rg, const double* planes, double2* tex, hipStream_t s) {
  const long long np = (long long)rg.nx * rg.ny;
  SW_LAUNCH(k_rays_pack, dim3((unsigned)((np + RAY_BLOCK - 1) / RAY_BLOCK)), dim3(RAY_BLOCK), 0, s, np, planes, tex);
}

void launch_rays_trace(const RayGrid& rg, const RayPhys& rp, bool blend_new, const double2* texo,
                       const double2* texn, double* xk, const double* sign, long long n, double duration,
                       int nsub, hipStream_t s) {
  const double h = duration / (double)nsub;
  if (blend_new)
    SW_LAUNCH(k_rays_trace<false>, ray_grid(n), dim3(RAY_BLOCK), 0, s, rg, rp, texn, texn, xk, sign, n, h, nsub);
  else
    SW_LAUNCH(k_rays_trace<true>, ray_grid(n), dim3(RAY_BLOCK), 0, s, rg, rp, texo, texn, xk, sign, n, h, nsub);
}

void launch_rays_sample(const RayGrid& rg, const double2* tex, const double* xk, long long n, double* U,
                        double* G, hipStream_t s) {
  SW_LAUNCH(k_rays_sample, ray_grid(n), dim3(RAY_BLOCK), 0, s, rg, tex, xk, n, U, G);
}

}  // namespace sw
