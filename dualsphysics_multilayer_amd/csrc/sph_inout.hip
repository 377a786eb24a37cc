// sph_inout.hip — inlet/outlet zones on CDNA4: the particle life cycle around the end-of-step
// divide and the ghost-node extrapolation.
//
// JSphCpuSingle::InOutComputeStep (JSphCpuSingle_InOut.cpp:146-223) runs in place of the
// end-of-step RunCellDivide of a case with <special><inout>:
//   * CreateListCpu (JSphInOut.cpp:801-831): a normal fluid particle that is not inout and lies
//     inside a zone that checks its input gets that zone's code + 16;
//   * ComputeStepCpu (JSphInOut.cpp:1036-1079): such a particle is removed (OUTPOS), converted
//     to an inout particle (code ^ 0x10) or made fluid again; an inout particle beyond the
//     zone's width (or above zsurf with `remove`) becomes OUTIGNORE — the sort drops it without
//     counting it as excluded —, one that crossed the zone's plane becomes fluid (CodeNewPart)
//     and, when refilling allows, is replaced by a new inlet particle one width behind it;
//   * the new particles (JSphInOut.cpp:1089-1108) are appended behind np in the ascending order
//     of the particles they replace, with the ids IdMax + 1 + k;
//   * RunCellDivide, then InOutUpdatePartsData (:228-255): SetAnalyticalDataCpu
//     (JSphInOut.cpp:906-959), Interaction_InOutExtrap (JSphCpu_InOut.cpp:55-465) and
//     UpdateVelrhopM1.
// Here the step pass is three launches with no host round trip, after the pattern of the
// periodic duplicates (sph_periodic.hip): k_inout_step (the rules; the new zone of every
// particle and per block of IB particles the number of new ones, from wave ballots),
// k_inout_scan (one block: exclusive prefix of the block counts, the capacity check, np, IdMax
// and the statistics), k_inout_create (ballot ranks inside a wave, the wave totals scanned in
// LDS, the block's prefix).  A pass that does not fit the capacity creates nothing and raises
// ERR_INOUT_FULL, which halts the run on the device like the other fatal flags.
// After the divide: k_inout_analytical (also lists the particles of the extrapolating zones),
// k_inout_extrap (one wave64 per listed particle; the partial sums of the lanes are reduced by
// a fixed butterfly, so two runs give the same bits whatever the order of the list) and
// k_inout_finish (VelrhopM1 and press of the inout particles, VelMax over the fluid: the
// divide's gather formed press and VelMax from the velocities it sorted).
#include <algorithm>

#include "sph_inout.hpp"

namespace sphx {

constexpr int IB = 256;            // particles per block of the step pass
constexpr unsigned IH_WORDS = 16;  // header words in front of the block counts
enum { IH_BASE = 0, IH_TOTAL = 1, IH_NUM = 2, IH_PINI = 3 };

size_t inout_scan_words(unsigned cap) { return size_t(IH_WORDS) + (size_t(cap) + IB - 1) / IB + 1; }

// JSphInOutZone::InZone (JSphInOutZone.cpp:372-381).
__device__ __forceinline__ bool in_zone(const InOutZoneDev& z, bool useboxlimit, float x, float y, float zz) {
  const bool box = z.boxmin[0] <= x && x <= z.boxmax[0] && z.boxmin[1] <= y && y <= z.boxmax[1] && z.boxmin[2] <= zz &&
                   zz <= z.boxmax[2];
  return (!useboxlimit || box) && (z.plane[0] * x + z.plane[1] * y + z.plane[2] * zz + z.plane[3]) < 0;
}

// CreateListCpu's classification and ComputeStepCpu's rules for particle p: writes its new
// code and returns the zone of the inlet particle to create for it (255: none).
__device__ __forceinline__ unsigned inout_rules(const InOutDev* __restrict__ io, const PartArrays& a, unsigned p,
                                                unsigned& removed) {
  typecode rcode = a.code[p];
  if (!CodeIsNormal(rcode) || !CodeIsFluid(rcode)) return 255u;
  const double2 pxy = a.posxy[p];
  const float x = float(pxy.x), y = float(pxy.y), z = float(a.posz[p]);
  if (!CodeIsFluidInout(rcode)) {
    if (io->checkfreelimit && !(x <= io->freemin[0] || io->freemax[0] <= x || z <= io->freemin[2] || io->freemax[2] <= z ||
                                y <= io->freemin[1] || io->freemax[1] <= y))
      return 255u;
    unsigned zone = 255u;
    for (int c = 0; c < io->nzones && zone == 255u; c++)
      if ((io->z[c].cfgzone & IO_CHECKINPUT) && in_zone(io->z[c], io->useboxlimit != 0, x, y, z)) zone = unsigned(c);
    if (zone == 255u) return 255u;
    rcode = typecode((rcode & ~CODE_MASKTYPEVALUE) | (CODE_TYPE_FLUID_INOUT | zone) | CODE_TYPE_FLUID_INOUTNUM);
  }
  const unsigned izone0 = rcode & CODE_TYPE_FLUID_INOUTMASK, izone = izone0 & CODE_TYPE_FLUID_INOUT015MASK;
  const InOutZoneDev& zo = io->z[izone < unsigned(io->nzones) ? izone : 0u];
  const unsigned cu = zo.cfgupdate;
  const bool zok = z <= zo.zsurf;
  const bool removezsurf = (cu & IO_REMOVEZSURF) != 0;
  typecode cod = 0;
  unsigned newiz = 255u;
  if (izone0 >= 16u) {  // normal fluid inside the zone
    if ((cu & IO_REMOVEINPUT) || (removezsurf && !zok)) {
      cod = CodeSetNormal(rcode) | CODE_OUTPOS;
      removed = 1u;
    } else {
      cod = (cu & IO_CONVERTINPUT) ? typecode(rcode ^ 0x10) : typecode(io->codenewpart);
    }
  } else {  // an inout particle
    const float pp = zo.plane[0] * x + zo.plane[1] * y + zo.plane[2] * z + zo.plane[3];
    const float displane = -(pp / sqrtf(zo.plane[0] * zo.plane[0] + zo.plane[1] * zo.plane[1] + zo.plane[2] * zo.plane[2]));
    if (displane > zo.width || (removezsurf && !zok)) {
      cod = CodeSetNormal(rcode) | CODE_OUTIGNORE;
      removed = 1u;
    } else if (displane < 0) {
      cod = typecode(io->codenewpart);
      if (!(cu & IO_REFILLADVANCED) && ((cu & IO_REFILLSPFULL) || zok)) newiz = izone;
    }
  }
  if (cod != 0) a.code[p] = cod;
  return newiz;
}

__global__ __launch_bounds__(IB) void k_inout_step(DevScalars* __restrict__ sc, const InOutDev* __restrict__ io,
                                                   PartArrays a, unsigned* __restrict__ scan,
                                                   unsigned char* __restrict__ newiz) {
  __shared__ unsigned wsum[IB / 64], wrem[IB / 64];
  if (halted(sc)) return;  // (uniform)
  const unsigned npb = sc->npb, np = sc->np;
  const unsigned num = np - npb;
  if (blockIdx.x * IB >= num) return;  // the whole block is past the fluid (uniform)
  const unsigned i = blockIdx.x * IB + threadIdx.x;
  unsigned nz = 255u, removed = 0u;
  if (i < num) {
    nz = inout_rules(io, a, npb + i, removed);
    newiz[npb + i] = (unsigned char)nz;
  }
  const unsigned long long bn = __ballot(nz != 255u), br = __ballot(removed != 0u);
  if ((threadIdx.x & 63) == 0) {
    wsum[threadIdx.x >> 6] = unsigned(__popcll(bn));
    wrem[threadIdx.x >> 6] = unsigned(__popcll(br));
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned t = 0u, r = 0u;
    for (int w = 0; w < IB / 64; w++) {
      t += wsum[w];
      r += wrem[w];
    }
    scan[IH_WORDS + blockIdx.x] = t;
    if (r) atomicAdd(&sc->io_removed, (unsigned long long)r);
  }
}

// One block: exclusive prefix of the block counts (in place), the capacity check and the new
// counts (Np, IdMax; JSphCpuSingle_InOut.cpp:204-209).
__global__ __launch_bounds__(1024) void k_inout_scan(DevScalars* __restrict__ sc, unsigned* __restrict__ scan,
                                                     unsigned cap) {
  __shared__ unsigned wtot[16];
  __shared__ unsigned carry, s_num;
  if (threadIdx.x == 0) {
    s_num = halted(sc) ? 0u : sc->np - sc->npb;
    carry = 0u;
  }
  __syncthreads();
  const unsigned num = s_num;
  const unsigned nblk = (num + IB - 1) / IB;
  unsigned* cnt = scan + IH_WORDS;
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (unsigned b0 = 0; b0 < nblk; b0 += 1024) {
    const unsigned b = b0 + threadIdx.x;
    const unsigned v = (b < nblk) ? cnt[b] : 0u;
    unsigned x = v;  // inclusive scan inside the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned y = (unsigned)__shfl_up((int)x, off, 64);
      if (lane >= unsigned(off)) x += y;
    }
    if (lane == 63) wtot[wave] = x;
    __syncthreads();
    unsigned wbase = 0u, all = 0u;
    for (unsigned w = 0; w < 16; w++) {
      if (w < wave) wbase += wtot[w];
      all += wtot[w];
    }
    const unsigned c = carry;
    if (b < nblk) cnt[b] = c + wbase + x - v;
    __syncthreads();
    if (threadIdx.x == 0) carry = c + all;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const unsigned np = sc->np;
    unsigned total = carry;
    if (total > cap - min(np, cap)) {  // does not fit: no particle is created
      sc->error_flags |= ERR_INOUT_FULL;
      total = 0u;
    }
    scan[IH_BASE] = np;
    scan[IH_TOTAL] = total;
    scan[IH_NUM] = num;
    scan[IH_PINI] = sc->npb;
    scan[IH_WORDS - 1] = sc->io_idmax + 1u;  // idnext
    sc->np = np + total;
    sc->io_idmax += total;
    sc->io_created += total;
  }
}

// The new inlet particle of every flagged one (JSphInOut.cpp:1094-1108).
__global__ __launch_bounds__(IB) void k_inout_create(const InOutDev* __restrict__ io, KConst K, PartArrays a,
                                                     const unsigned* __restrict__ scan,
                                                     const unsigned char* __restrict__ newiz, unsigned cap) {
  __shared__ unsigned wsum[IB / 64];
  const unsigned base = scan[IH_BASE], total = scan[IH_TOTAL], num = scan[IH_NUM], pini = scan[IH_PINI];
  if (!total || blockIdx.x * IB >= num) return;  // nothing to create (or it did not fit); uniform
  const unsigned idnext = scan[IH_WORDS - 1];
  const unsigned i = blockIdx.x * IB + threadIdx.x;
  const unsigned p = pini + i;
  const unsigned nz = (i < num) ? unsigned(newiz[p]) : 255u;
  const unsigned long long bn = __ballot(nz != 255u);
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned rank = unsigned(__popcll(bn & ((1ull << lane) - 1ull)));
  if (lane == 0) wsum[wave] = unsigned(__popcll(bn));
  __syncthreads();
  unsigned k = scan[IH_WORDS + blockIdx.x] + rank;
  for (unsigned w = 0; w < wave; w++) k += wsum[w];
  const unsigned p2 = base + k;
  // (the scan admitted base + total <= cap; the guard keeps a disagreement out of memory)
  if (nz == 255u || k >= total || p2 >= cap) return;
  const InOutZoneDev& zo = io->z[nz];
  const double dis = double(zo.width);
  const double2 pxy = a.posxy[p];
  const double rx = pxy.x - nc(dis * double(zo.dir[0])), ry = pxy.y - nc(dis * double(zo.dir[1])),
               rz = a.posz[p] - nc(dis * double(zo.dir[2]));
  typecode rcode = typecode((io->codenewpart & ~CODE_MASKTYPEVALUE) | (CODE_TYPE_FLUID_INOUT | nz));
  a.code[p2] = rcode;
  update_pos(K, rx, ry, rz, 0., 0., 0., false, p2, a, &rcode);
  a.idp[p2] = idnext + k;
  a.velrhop[p2] = make_float4(0.f, 0.f, 0.f, 1000.f);
  if (a.velrhopm1) a.velrhopm1[p2] = make_float4(0.f, 0.f, 0.f, 1000.f);
}

void launch_inout_step(hipStream_t stm, unsigned cap, DevScalars* sc, const InOutDev* io, const KConst& K,
                       const PartArrays& a, unsigned* scan, unsigned char* newiz) {
  const unsigned nb = (cap + IB - 1) / IB;
  hipLaunchKernelGGL(k_inout_step, dim3(nb), dim3(IB), 0, stm, sc, io, a, scan, newiz);
  hipLaunchKernelGGL(k_inout_scan, dim3(1), dim3(1024), 0, stm, sc, scan, cap);
  hipLaunchKernelGGL(k_inout_create, dim3(nb), dim3(IB), 0, stm, io, K, a, scan, newiz, cap);
}

// JSphInOutZone::CalcVel (JSphInOutZone.cpp:352-367).
__device__ __forceinline__ float calc_vel(unsigned vprof, const float* v, double posz) {
  if (vprof == IO_VELP_LINEAR) return v[0] * float(posz) + v[1];
  if (vprof == IO_VELP_PARABOLIC) return v[0] * float(posz) * float(posz) + v[1] * float(posz) + v[2];
  return v[0];
}

// SetAnalyticalDataCpu (JSphInOut.cpp:906-959) for every inout particle (normal or not out:
// CreateListSimpleCpu, :780-795); the particles of a zone that extrapolates are listed.
__global__ __launch_bounds__(256) void k_inout_analytical(DevScalars* __restrict__ sc, const InOutDev* __restrict__ io,
                                                          KConst K, PartArrays a, unsigned* __restrict__ list) {
  const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned lane = threadIdx.x & 63;
  typecode rcode = 0;
  bool inout = false;
  if (p >= sc->npb && p < sc->np) {
    rcode = a.code[p];
    inout = CodeSpecial(rcode) < CODE_OUTIGNORE && CodeIsFluidInout(rcode);
  }
  const unsigned izone = rcode & CODE_TYPE_FLUID_INOUTMASK;
  const InOutZoneDev& zo = io->z[izone < unsigned(io->nzones) ? izone : 0u];
  const unsigned cfg = zo.cfgzone;
  const unsigned rmode = cfg & IO_RHOP_MASK, vmode = cfg & IO_VELM_MASK;
  const bool listed = inout && (rmode == IO_RHOP_EXTRAPOLATED || vmode == IO_VELM_EXTRAPOLATED);
  // one atomic per wave for the count and for the list's slots (ballot ranks inside the wave)
  const unsigned long long bi = __ballot(inout), bl = __ballot(listed);
  if (bi) {  // (uniform)
    unsigned slot = 0u;
    if (lane == 0) {
      atomicAdd(&sc->io_count, unsigned(__popcll(bi)));
      if (bl) slot = atomicAdd(&sc->io_nlist, unsigned(__popcll(bl)));
    }
    slot = unsigned(__shfl(int(slot), 0, 64));
    if (listed) list[slot + unsigned(__popcll(bl & ((1ull << lane) - 1ull)))] = p;
  }
  if (!inout || (rmode == IO_RHOP_EXTRAPOLATED && vmode == IO_VELM_EXTRAPOLATED)) return;
  const double posz = a.posz[p];
  float4 v = a.velrhop[p];
  if (rmode == IO_RHOP_CONSTANT) v.w = K.rhopzero;
  if (rmode == IO_RHOP_HYDROSTATIC) {
    const float depth = float(double(zo.zsurf) - posz);
    const float rh = 1.f + io->coefhydro * depth;
    const float frhop = powf(rh, 1.f / K.gamma);
    v.w = K.rhopzero * (frhop < 1.f ? 1.f : frhop);  // no density below rhopzero (suction)
  }
  if (vmode == IO_VELM_FIXED) {
    float vel = 0.f;
    if (!(zo.cfgupdate & IO_REFILLSPFULL) || posz <= double(zo.zsurf)) vel = calc_vel(cfg & IO_VELP_MASK, zo.vel0, posz);
    v.x = vel * zo.dir[0];
    v.y = vel * zo.dir[1];
    v.z = vel * zo.dir[2];
  }
  a.velrhop[p] = v;
}

// ---- Interaction_InOutExtrap (JSphCpu_InOut.cpp:55-237 all double, :243-422 float sums) --------
template <class T> __device__ __forceinline__ T wsum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Determinant and inverse of the correction matrix (FunctionsMath.h:91-93, 157-171, 186-199, 260-282).
template <class M> __device__ __forceinline__ M det3(const M* d) {
  return d[0] * d[4] * d[8] + d[1] * d[5] * d[6] + d[2] * d[3] * d[7] - d[6] * d[4] * d[2] - d[7] * d[5] * d[0] -
         d[8] * d[3] * d[1];
}
template <class M> __device__ __forceinline__ void inv3(const M* d, M det, M* inv) {
  inv[0] = (d[4] * d[8] - d[5] * d[7]) / det;
  inv[1] = -(d[1] * d[8] - d[2] * d[7]) / det;
  inv[2] = (d[1] * d[5] - d[2] * d[4]) / det;
  inv[3] = -(d[3] * d[8] - d[5] * d[6]) / det;
  inv[4] = (d[0] * d[8] - d[2] * d[6]) / det;
  inv[5] = -(d[0] * d[5] - d[2] * d[3]) / det;
  inv[6] = (d[3] * d[7] - d[4] * d[6]) / det;
  inv[7] = -(d[0] * d[7] - d[1] * d[6]) / det;
  inv[8] = (d[0] * d[4] - d[1] * d[3]) / det;
}
// d[4 r + c] = a(r+1)(c+1)
template <class M> __device__ __forceinline__ M det4(const M* d) {
  return d[3] * d[6] * d[9] * d[12] - d[2] * d[7] * d[9] * d[12] - d[3] * d[5] * d[10] * d[12] + d[1] * d[7] * d[10] * d[12] +
         d[2] * d[5] * d[11] * d[12] - d[1] * d[6] * d[11] * d[12] - d[3] * d[6] * d[8] * d[13] + d[2] * d[7] * d[8] * d[13] +
         d[3] * d[4] * d[10] * d[13] - d[0] * d[7] * d[10] * d[13] - d[2] * d[4] * d[11] * d[13] + d[0] * d[6] * d[11] * d[13] +
         d[3] * d[5] * d[8] * d[14] - d[1] * d[7] * d[8] * d[14] - d[3] * d[4] * d[9] * d[14] + d[0] * d[7] * d[9] * d[14] +
         d[1] * d[4] * d[11] * d[14] - d[0] * d[5] * d[11] * d[14] - d[2] * d[5] * d[8] * d[15] + d[1] * d[6] * d[8] * d[15] +
         d[2] * d[4] * d[9] * d[15] - d[0] * d[6] * d[9] * d[15] - d[1] * d[4] * d[10] * d[15] + d[0] * d[5] * d[10] * d[15];
}
template <class M> __device__ __forceinline__ void inv4(const M* d, M det, M* inv) {
  const M a11 = d[0], a12 = d[1], a13 = d[2], a14 = d[3], a21 = d[4], a22 = d[5], a23 = d[6], a24 = d[7], a31 = d[8],
          a32 = d[9], a33 = d[10], a34 = d[11], a41 = d[12], a42 = d[13], a43 = d[14], a44 = d[15];
  inv[0] = (a22 * (a33 * a44 - a34 * a43) + a23 * (a34 * a42 - a32 * a44) + a24 * (a32 * a43 - a33 * a42)) / det;
  inv[4] = (a21 * (a34 * a43 - a33 * a44) + a23 * (a31 * a44 - a34 * a41) + a24 * (a33 * a41 - a31 * a43)) / det;
  inv[8] = (a21 * (a32 * a44 - a34 * a42) + a22 * (a34 * a41 - a31 * a44) + a24 * (a31 * a42 - a32 * a41)) / det;
  inv[12] = (a21 * (a33 * a42 - a32 * a43) + a22 * (a31 * a43 - a33 * a41) + a23 * (a32 * a41 - a31 * a42)) / det;
  inv[1] = (a12 * (a34 * a43 - a33 * a44) + a13 * (a32 * a44 - a34 * a42) + a14 * (a33 * a42 - a32 * a43)) / det;
  inv[5] = (a11 * (a33 * a44 - a34 * a43) + a13 * (a34 * a41 - a31 * a44) + a14 * (a31 * a43 - a33 * a41)) / det;
  inv[9] = (a11 * (a34 * a42 - a32 * a44) + a12 * (a31 * a44 - a34 * a41) + a14 * (a32 * a41 - a31 * a42)) / det;
  inv[13] = (a11 * (a32 * a43 - a33 * a42) + a12 * (a33 * a41 - a31 * a43) + a13 * (a31 * a42 - a32 * a41)) / det;
  inv[2] = (a12 * (a23 * a44 - a24 * a43) + a13 * (a24 * a42 - a22 * a44) + a14 * (a22 * a43 - a23 * a42)) / det;
  inv[6] = (a11 * (a24 * a43 - a23 * a44) + a13 * (a21 * a44 - a24 * a41) + a14 * (a23 * a41 - a21 * a43)) / det;
  inv[10] = (a11 * (a22 * a44 - a24 * a42) + a12 * (a24 * a41 - a21 * a44) + a14 * (a21 * a42 - a22 * a41)) / det;
  inv[14] = (a11 * (a23 * a42 - a22 * a43) + a12 * (a21 * a43 - a23 * a41) + a13 * (a22 * a41 - a21 * a42)) / det;
  inv[3] = (a12 * (a24 * a33 - a23 * a34) + a13 * (a22 * a34 - a24 * a32) + a14 * (a23 * a32 - a22 * a33)) / det;
  inv[7] = (a11 * (a23 * a34 - a24 * a33) + a13 * (a24 * a31 - a21 * a34) + a14 * (a21 * a33 - a23 * a31)) / det;
  inv[11] = (a11 * (a24 * a32 - a22 * a34) + a12 * (a21 * a34 - a24 * a31) + a14 * (a22 * a31 - a21 * a32)) / det;
  inv[15] = (a11 * (a22 * a33 - a23 * a32) + a12 * (a23 * a31 - a21 * a33) + a13 * (a21 * a32 - a22 * a31)) / det;
}

// One wave per listed inout particle.  S: the type of the sums of rho, grad rho, v and grad v
// (and of the pair terms), M: the type of the correction matrix.  Mode 1 (fast-single): float,
// float; mode 2 (single): float, double; mode 3 (double): double, double.  SIM2D: the 3x3 matrix
// in (1, x, z), else the 4x4 in (1, x, y, z).
template <class S, class M, bool SIM2D>
__global__ __launch_bounds__(256) void k_inout_extrap(const DevScalars* __restrict__ sc, const InOutDev* __restrict__ io,
                                                      KConst K, DivGrid g, PartArrays a, const unsigned* __restrict__ bc,
                                                      const unsigned* __restrict__ list) {
  constexpr int ND = SIM2D ? 3 : 4;  // matrix order
  const unsigned nlist = sc->io_nlist;
  const unsigned lane = threadIdx.x & 63;
  const unsigned nwaves = gridDim.x * (blockDim.x >> 6);
  for (unsigned w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w < nlist; w += nwaves) {
    const unsigned p1 = list[w];
    const typecode code1 = a.code[p1];
    const unsigned izone = code1 & CODE_TYPE_FLUID_INOUTMASK;
    const InOutZoneDev& zo = io->z[izone < unsigned(io->nzones) ? izone : 0u];
    const bool computerhop = (zo.cfgzone & IO_RHOP_MASK) == IO_RHOP_EXTRAPOLATED;
    const bool computevel = (zo.cfgzone & IO_VELM_MASK) == IO_VELM_EXTRAPOLATED;
    // the ghost node: the particle mirrored in the zone's plane (JSphCpu_InOut.cpp:76-79)
    const double2 pxy1 = a.posxy[p1];
    const double pz1 = a.posz[p1];
    const double pa = double(zo.plane[0]), pb = double(zo.plane[1]), pc = double(zo.plane[2]), pd = double(zo.plane[3]);
    const double displane = fabs((pa * pxy1.x + pb * pxy1.y + pc * pz1 + pd) / sqrt(pa * pa + pb * pb + pc * pc)) * 2;
    const double gx = pxy1.x + displane * double(zo.dir[0]), gy = pxy1.y + displane * double(zo.dir[1]),
                 gz = pz1 + displane * double(zo.dir[2]);
    S rhop = 0, grx = 0, gry = 0, grz = 0, vx = 0, vy = 0, vz = 0;
    S gv[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    M ac[ND * ND];
#pragma unroll
    for (int k = 0; k < ND * ND; k++) ac[k] = 0;
    // nsearch::Init(posp1, false, dvd) (JCellSearch_inline.h:54-69)
    const int cx = cell_of(gx - K.map_realposmin_x, K.scelld), cy = cell_of(gy - K.map_realposmin_y, K.scelld),
              cz = cell_of(gz - K.map_realposmin_z, K.scelld);
    if (cx >= 0 && cy >= 0 && cz >= 0 && cx < g.ncx && cy < g.ncy && cz < g.ncz) {
      const int s = K.scelldiv;
      const int cxini = cx - min(cx, s), cxfin = cx + min(g.ncx - cx - 1, s) + 1;
      const int yini = cy - min(cy, s), yfin = cy + min(g.ncy - cy - 1, s) + 1;
      const int zini = cz - min(cz, s), zfin = cz + min(g.ncz - cz - 1, s) + 1;
      for (int z = zini; z < zfin; z++)
        for (int y = yini; y < yfin; y++) {
          const unsigned v = g.boxfluid + g.nsheet * unsigned(z) + unsigned(g.ncx) * unsigned(y);
          const unsigned pini = bc[v + unsigned(cxini)], pfin = bc[v + unsigned(cxfin)];
          for (unsigned p2 = pini + lane; p2 < pfin; p2 += 64) {
            const double2 pxy2 = a.posxy[p2];
            const S drx = S(gx - pxy2.x), dry = S(gy - pxy2.y), drz = S(gz - a.posz[p2]);
            const S rr2 = drx * drx + dry * dry + drz * drz;
            if (rr2 <= S(K.kernelsize2) && rr2 >= S(ALMOSTZERO) && CodeIsFluidNotInout(a.code[p2])) {
              // GetKernelWendland_WabFac (FunSphKernel.h:226-234), in float in every mode
              const float rad = sqrtf(float(rr2));
              const float qq = rad / K.kernelh;
              const float wqq1 = 1.f - 0.5f * qq;
              const float wqq2 = wqq1 * wqq1;
              const float fac = K.bwen * qq * wqq2 * wqq1 / rad;
              const float wqq = qq + qq + 1.f;
              const S wab = S(K.awen * wqq * wqq2 * wqq2);
              const S frx = S(fac) * drx, fry = S(fac) * dry, frz = S(fac) * drz;
              const float4 v2 = a.velrhop[p2];
              const S massp2 = S(K.massfluid);
              const S volp2 = massp2 / S(v2.w);
              rhop += massp2 * wab;
              grx += massp2 * frx;
              gry += massp2 * fry;
              grz += massp2 * frz;
              const S vwab = wab * volp2, vfrx = frx * volp2, vfry = fry * volp2, vfrz = frz * volp2;
              if (computevel) {
                vx += vwab * S(v2.x);
                vy += vwab * S(v2.y);
                vz += vwab * S(v2.z);
                gv[0] += vfrx * S(v2.x);
                gv[1] += vfry * S(v2.x);
                gv[2] += vfrz * S(v2.x);
                gv[3] += vfrx * S(v2.y);
                gv[4] += vfry * S(v2.y);
                gv[5] += vfrz * S(v2.y);
                gv[6] += vfrx * S(v2.z);
                gv[7] += vfry * S(v2.z);
                gv[8] += vfrz * S(v2.z);
              }
              if (SIM2D) {
                ac[0] += M(vwab); ac[1] += M(drx * vwab); ac[2] += M(drz * vwab);
                ac[3] += M(vfrx); ac[4] += M(drx * vfrx); ac[5] += M(drz * vfrx);
                ac[6] += M(vfrz); ac[7] += M(drx * vfrz); ac[8] += M(drz * vfrz);
              } else {
                ac[0] += M(vwab); ac[1] += M(drx * vwab); ac[2] += M(dry * vwab); ac[3] += M(drz * vwab);
                ac[4] += M(vfrx); ac[5] += M(drx * vfrx); ac[6] += M(dry * vfrx); ac[7] += M(drz * vfrx);
                ac[8] += M(vfry); ac[9] += M(drx * vfry); ac[10] += M(dry * vfry); ac[11] += M(drz * vfry);
                ac[12] += M(vfrz); ac[13] += M(drx * vfrz); ac[14] += M(dry * vfrz); ac[15] += M(drz * vfrz);
              }
            }
          }
        }
    }
    rhop = wsum(rhop); grx = wsum(grx); gry = wsum(gry); grz = wsum(grz);
    vx = wsum(vx); vy = wsum(vy); vz = wsum(vz);
#pragma unroll
    for (int k = 0; k < 9; k++) gv[k] = wsum(gv[k]);
#pragma unroll
    for (int k = 0; k < ND * ND; k++) ac[k] = wsum(ac[k]);
    if (lane != 0) continue;
    float4 vf = a.velrhop[p1];
    const S dx = S(pxy1.x - gx), dy = S(pxy1.y - gy), dz = S(pz1 - gz);
    const M determ = SIM2D ? det3(ac) : det4(ac);
    if (fabs(double(determ)) >= double(io->determlimit)) {
      M in[ND * ND];
      if (SIM2D) inv3(ac, determ, in);
      else inv4(ac, determ, in);
      if (SIM2D) {
        if (computerhop) {
          const S rg = S(in[0] * M(rhop) + in[1] * M(grx) + in[2] * M(grz));
          const S ax = -S(in[3] * M(rhop) + in[4] * M(grx) + in[5] * M(grz));
          const S az = -S(in[6] * M(rhop) + in[7] * M(grx) + in[8] * M(grz));
          vf.w = float(rg + ax * dx + az * dz);
        }
        if (computevel) {
          const S ux = S(in[0] * M(vx) + in[1] * M(gv[0]) + in[2] * M(gv[2]));
          const S uz = S(in[0] * M(vz) + in[1] * M(gv[6]) + in[2] * M(gv[8]));
          const S a11 = -S(in[3] * M(vx) + in[4] * M(gv[0]) + in[5] * M(gv[2]));
          const S a13 = -S(in[3] * M(vz) + in[4] * M(gv[6]) + in[5] * M(gv[8]));
          const S a31 = -S(in[6] * M(vx) + in[7] * M(gv[0]) + in[8] * M(gv[2]));
          const S a33 = -S(in[6] * M(vz) + in[7] * M(gv[6]) + in[8] * M(gv[8]));
          vf.x = float(ux + a11 * dx + a31 * dz);
          vf.z = float(uz + a13 * dx + a33 * dz);
          vf.y = 0.f;
        }
      } else {
        if (computerhop) {
          const S rg = S(in[0] * M(rhop) + in[1] * M(grx) + in[2] * M(gry) + in[3] * M(grz));
          const S ax = -S(in[4] * M(rhop) + in[5] * M(grx) + in[6] * M(gry) + in[7] * M(grz));
          const S ay = -S(in[8] * M(rhop) + in[9] * M(grx) + in[10] * M(gry) + in[11] * M(grz));
          const S az = -S(in[12] * M(rhop) + in[13] * M(grx) + in[14] * M(gry) + in[15] * M(grz));
          vf.w = float(rg + ax * dx + ay * dy + az * dz);
        }
        if (computevel) {
          const M q[3] = {M(vx), M(vy), M(vz)};
          S ug[3], ga[3][3];  // ga[r][c]: gradient row r (x, y, z) of component c
#pragma unroll
          for (int c = 0; c < 3; c++) {
            ug[c] = S(in[0] * q[c] + in[1] * M(gv[3 * c]) + in[2] * M(gv[3 * c + 1]) + in[3] * M(gv[3 * c + 2]));
#pragma unroll
            for (int r = 0; r < 3; r++)
              ga[r][c] = -S(in[4 * (r + 1)] * q[c] + in[4 * (r + 1) + 1] * M(gv[3 * c]) + in[4 * (r + 1) + 2] * M(gv[3 * c + 1]) +
                            in[4 * (r + 1) + 3] * M(gv[3 * c + 2]));
          }
          vf.x = float(ug[0] + ga[0][0] * dx + ga[1][0] * dy + ga[2][0] * dz);
          vf.y = float(ug[1] + ga[0][1] * dx + ga[1][1] * dy + ga[2][1] * dz);
          vf.z = float(ug[2] + ga[0][2] * dx + ga[1][2] * dy + ga[2][2] * dz);
        }
      }
    } else if (ac[0] > 0) {  // the zeroth-order values
      if (computerhop) vf.w = float(M(rhop) / ac[0]);
      if (computevel) {
        vf.x = float(M(vx) / ac[0]);
        vf.z = float(M(vz) / ac[0]);
        vf.y = SIM2D ? 0.f : float(M(vy) / ac[0]);
      }
    }
    a.velrhop[p1] = vf;
  }
}

// UpdateVelrhopM1 (JSphInOut.cpp) and the divide's press (eos_press, as sph_divide.hip gather_store) of the
// inout particles from their new velocity and density; VelMax (CalcVelMaxOmp) over the fluid,
// or every particle with DtAllParticles, in slots the caller cleared.
__global__ __launch_bounds__(256) void k_inout_finish(DevScalars* __restrict__ sc, KConst K, PartArrays a,
                                                      float* __restrict__ press, int withm1) {
  const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned np = sc->np, npb = sc->npb;
  float v2 = 0.f;
  if (p < np) {
    const float4 v = a.velrhop[p];
    if (p >= npb || K.dtallp) v2 = v.x * v.x + v.y * v.y + v.z * v.z;
    if (p >= npb) {
      const typecode rcode = a.code[p];
      if (CodeSpecial(rcode) < CODE_OUTIGNORE && CodeIsFluidInout(rcode)) {
        if (withm1) a.velrhopm1[p] = v;
        press[p] = eos_press(K.cteb, K.ovrhopzero, K.gamma, integer_gamma_of(K.gamma), v.w);
      }
    }
  }
  block_max_atomic(sc, RED_VELMAX2, v2);
}

__global__ void k_inout_begin_parts(DevScalars* __restrict__ sc) {
  if (threadIdx.x < RED_SLOTS) sc->red[RED_VELMAX2][threadIdx.x] = 0u;
  if (threadIdx.x == 0) {
    sc->io_count = 0u;
    sc->io_nlist = 0u;
  }
}

void launch_inout_parts(hipStream_t stm, unsigned cap, DevScalars* sc, const InOutDev* io, const InOutDev& ioh,
                        const KConst& K, const DivGrid& g, const PartArrays& a, const unsigned* begincell, float* press,
                        unsigned* list, bool withm1) {
  const unsigned nb = (cap + 255) / 256;
  hipLaunchKernelGGL(k_inout_begin_parts, dim3(1), dim3(64), 0, stm, sc);
  hipLaunchKernelGGL(k_inout_analytical, dim3(nb), dim3(256), 0, stm, sc, io, K, a, list);
  bool extrap = false;
  for (int c = 0; c < ioh.nzones; c++)
    extrap = extrap || (ioh.z[c].cfgzone & IO_RHOP_MASK) == IO_RHOP_EXTRAPOLATED ||
             (ioh.z[c].cfgzone & IO_VELM_MASK) == IO_VELM_EXTRAPOLATED;
  if (extrap) {
    // waves stride over the list: the grid covers a list of up to 4096 particles in one round
    const unsigned ne = std::min(nb, 1024u);
    const bool s2 = K.sim2d != 0;
#define SPH_K_EXTRAP(S, M)                                                                                       \
  if (s2) hipLaunchKernelGGL((k_inout_extrap<S, M, true>), dim3(ne), dim3(256), 0, stm, sc, io, K, g, a, begincell, list); \
  else hipLaunchKernelGGL((k_inout_extrap<S, M, false>), dim3(ne), dim3(256), 0, stm, sc, io, K, g, a, begincell, list)
    if (ioh.extrapmode >= 3) { SPH_K_EXTRAP(double, double); }
    else if (ioh.extrapmode == 2) { SPH_K_EXTRAP(float, double); }
    else { SPH_K_EXTRAP(float, float); }
#undef SPH_K_EXTRAP
  }
  hipLaunchKernelGGL(k_inout_finish, dim3(nb), dim3(256), 0, stm, sc, K, a, press, int(withm1));
}

__global__ __launch_bounds__(256) void k_inout_acemax(DevScalars* __restrict__ sc, const typecode* __restrict__ code,
                                                      const float4* __restrict__ arace) {
  const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
  float ace2 = 0.f;
  if (p >= sc->npb && p < sc->np) {
    const typecode c = code[p];
    if (CodeIsNormal(c) && !CodeIsFluidInout(c)) {
      const float4 ra = arace[p];
      ace2 = ra.x * ra.x + ra.y * ra.y + ra.z * ra.z;
    }
  }
  block_max_atomic(sc, RED_ACEMAX2, ace2);
}

void launch_inout_acemax(hipStream_t stm, unsigned cap, DevScalars* sc, const typecode* code, const float4* arace) {
  hipLaunchKernelGGL(k_inout_acemax, dim3((cap + 255) / 256), dim3(256), 0, stm, sc, code, arace);
}

}  // namespace sphx
