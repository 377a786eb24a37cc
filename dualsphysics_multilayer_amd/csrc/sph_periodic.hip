// sph_periodic.hip — periodic boundaries on CDNA4: the duplicates of every divide.
//
// JSphCpuSingle::RunPeriodic (JSphCpuSingle.cpp:361-431) runs before every divide of a case with
// PeriActive != 0:
//   * the duplicates of the previous divide become CODE_OUTIGNORE: the sort puts them in the
//     out-ignore boxes behind np, where they are neither counted as excluded nor kept;
//   * per particle type (boundary, then fluid), per periodic axis (X, Y, Z), per block (first the
//     duplicates of that type made so far in this call — that makes the corner images of two
//     periodic axes —, then the type's original particles) PeriodicMakeList (:191-222) lists
//     every normal or periodic particle whose pos + inc lies in [Map_PosMin, Map_PosMax), and once
//     more with the inverse mark when pos - inc does: ascending index, +inc before -inc;
//   * PeriodicDuplicateVerlet / Symplectic (:239-321) copy the listed particles to the end of
//     the arrays: displaced position, dcell from DomPosMin, same idp, code | CODE_PERIODIC, and
//     every other array the divide gathers.
// The duplicates are ordinary particles of the edge cells afterwards: the (stable) sort puts
// them behind the particles their cell already held, in list order, so the interaction sums
// its neighbours in the reference's order.
//
// Here a pass is three launches with no host round trip: k_peri_count (per block of PB
// particles the number of list entries, from wave ballots), k_peri_scan (one block: exclusive
// prefix of the block counts, the capacity check, sc->np and the type's count), k_peri_write
// (the entries of each block in order: ballot ranks inside a wave, the wave totals scanned in
// LDS, the block's prefix; each entry copies its particle).  The list itself is never stored.
// A pass that does not fit the capacity writes nothing and raises ERR_PERI_FULL, which halts
// the run on the device like the other fatal flags.
#include "sph_kernels.hpp"

namespace sphx {

constexpr int PB = 256;           // particles per block of a pass
constexpr unsigned PH_WORDS = 16; // header words in front of the block counts
// header: [0] np at the start of RunPeriodic, [1] npb there, and of the pass in flight:
// [2] first particle examined, [3] particles examined, [4] base (np before it), [5] entries
// written (0 when they did not fit)
enum { PH_NP0 = 0, PH_NPB0 = 1, PH_PINI = 2, PH_NUM = 3, PH_BASE = 4, PH_TOTAL = 5 };

size_t peri_scan_words(unsigned cap) { return size_t(PH_WORDS) + (size_t(cap) + PB - 1) / PB + 1; }

// Old duplicates -> CODE_OUTIGNORE (JSphCpuSingle.cpp:367-370); the counts of this call start.
__global__ __launch_bounds__(256) void k_peri_mark(DevScalars* __restrict__ sc, typecode* __restrict__ code,
                                                   unsigned* __restrict__ hdr) {
  const unsigned np = sc->np;
  const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p == 0) {
    hdr[PH_NP0] = np;
    hdr[PH_NPB0] = sc->npb;
    sc->npbper = 0u;
    sc->npfper = 0u;
  }
  if (p >= np) return;
  const typecode c = code[p];
  if (CodeSpecial(c) == CODE_PERIODIC) code[p] = CodeSetNormal(c) | CODE_OUTIGNORE;
}

// The particles a pass examines (RunPeriodic's pini2 / num2): block 0 the duplicates of the
// type made so far (the last nper before np), block 1 its originals.
__device__ __forceinline__ void peri_range(const DevScalars* __restrict__ sc, const unsigned* __restrict__ hdr,
                                           int type, int block, unsigned& pini, unsigned& num) {
  const unsigned np0 = hdr[PH_NP0], npb0 = hdr[PH_NPB0];
  if (block == 0) {
    const unsigned nper = type ? sc->npfper : sc->npbper;
    pini = sc->np - nper;
    num = nper;
  } else {
    pini = type ? npb0 : 0u;
    num = type ? np0 - npb0 : npb0;
  }
}

// PeriodicMakeList's test for particle p2 (JSphCpuSingle.cpp:202-212): bit 0 the +inc entry,
// bit 1 the -inc (inverse) entry.
__device__ __forceinline__ unsigned peri_flags(const PeriConst& P, int axis, const PartArrays& a, unsigned p2) {
  if (CodeSpecial(a.code[p2]) > CODE_PERIODIC) return 0u;
  const double2 pxy = a.posxy[p2];
  const double pz = a.posz[p2];
  const double ix = P.inc[axis][0], iy = P.inc[axis][1], iz = P.inc[axis][2];
  unsigned f = 0u;
  {
    const double x = pxy.x + ix, y = pxy.y + iy, z = pz + iz;
    if (P.mapposmin[0] <= x && P.mapposmin[1] <= y && P.mapposmin[2] <= z && x < P.mapposmax[0] &&
        y < P.mapposmax[1] && z < P.mapposmax[2])
      f |= 1u;
  }
  {
    const double x = pxy.x - ix, y = pxy.y - iy, z = pz - iz;
    if (P.mapposmin[0] <= x && P.mapposmin[1] <= y && P.mapposmin[2] <= z && x < P.mapposmax[0] &&
        y < P.mapposmax[1] && z < P.mapposmax[2])
      f |= 2u;
  }
  return f;
}

__global__ __launch_bounds__(PB) void k_peri_count(const DevScalars* __restrict__ sc, PeriConst P, PartArrays a,
                                                   unsigned* __restrict__ scan, int type, int axis, int block) {
  __shared__ unsigned wsum[PB / 64];
  unsigned pini, num;
  peri_range(sc, scan, type, block, pini, num);
  const unsigned i = blockIdx.x * PB + threadIdx.x;
  if (blockIdx.x * PB >= num) return;  // the whole block is past the range (uniform)
  const unsigned f = (i < num) ? peri_flags(P, axis, a, pini + i) : 0u;
  const unsigned long long bp = __ballot(f & 1u), bm = __ballot(f & 2u);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = unsigned(__popcll(bp) + __popcll(bm));
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned t = 0u;
    for (int w = 0; w < PB / 64; w++) t += wsum[w];
    scan[PH_WORDS + blockIdx.x] = t;
  }
}

// One block: exclusive prefix of the pass's block counts (in place), the capacity check and
// the new counts (Np += count; NpbPer / NpfPer += count, JSphCpuSingle.cpp:421-424).
__global__ __launch_bounds__(1024) void k_peri_scan(DevScalars* __restrict__ sc, unsigned* __restrict__ scan, int type,
                                                    int block, unsigned cap) {
  __shared__ unsigned wtot[16];
  __shared__ unsigned carry, s_pini, s_num;
  // thread 0 reads the range and, at the end, moves the counts it depends on: every other
  // thread takes it from LDS, so none reads sc after that
  if (threadIdx.x == 0) {
    unsigned a, b;
    peri_range(sc, scan, type, block, a, b);
    s_pini = a;
    s_num = b;
    carry = 0u;
  }
  __syncthreads();
  const unsigned pini = s_pini, num = s_num;
  const unsigned nblk = (num + PB - 1) / PB;
  unsigned* cnt = scan + PH_WORDS;
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
    if (total > cap - min(np, cap)) {  // does not fit: nothing is written past the capacity
      sc->error_flags |= ERR_PERI_FULL;
      total = 0u;
    }
    scan[PH_PINI] = pini;
    scan[PH_NUM] = num;
    scan[PH_BASE] = np;
    scan[PH_TOTAL] = total;
    sc->np = np + total;
    if (type) sc->npfper += total;
    else sc->npbper += total;
  }
}

// PeriodicDuplicatePos + PeriodicDuplicateVerlet / Symplectic (JSphCpuSingle.cpp:239-321) for
// entry `pnew` made from particle `pc`.
template <bool WITHM1, bool WITHPRE>
__device__ __forceinline__ void peri_duplicate(const PeriConst& P, const KConst& K, int axis, const PartArrays& a,
                                               unsigned pnew, unsigned pc, bool inverse) {
  const double2 pxy = a.posxy[pc];
  const double pz = a.posz[pc];
  const double dx = P.inc[axis][0], dy = P.inc[axis][1], dz = P.inc[axis][2];
  const double x = pxy.x + (inverse ? -dx : dx), y = pxy.y + (inverse ? -dy : dy), z = pz + (inverse ? -dz : dz);
  unsigned cx = unsigned((x - P.domposmin[0]) / K.scelld);
  unsigned cy = unsigned((y - P.domposmin[1]) / K.scelld);
  unsigned cz = unsigned((z - P.domposmin[2]) / K.scelld);
  cx = min(cx, P.cellmax[0]);
  cy = min(cy, P.cellmax[1]);
  cz = min(cz, P.cellmax[2]);
  a.posxy[pnew] = make_double2(x, y);
  a.posz[pnew] = z;
  a.dcell[pnew] = DcelCell(K.domcellcode, cx, cy, cz);
  a.idp[pnew] = a.idp[pc];
  a.code[pnew] = CodeSetNormal(a.code[pc]) | CODE_PERIODIC;
  a.velrhop[pnew] = a.velrhop[pc];
  if (WITHM1) a.velrhopm1[pnew] = a.velrhopm1[pc];
  if (WITHPRE) {
    a.posxypre[pnew] = a.posxypre[pc];
    a.poszpre[pnew] = a.poszpre[pc];
    a.velrhoppre[pnew] = a.velrhoppre[pc];
  }
}

template <bool WITHM1, bool WITHPRE>
__global__ __launch_bounds__(PB) void k_peri_write(PeriConst P, KConst K, PartArrays a,
                                                   const unsigned* __restrict__ scan, int axis, unsigned cap) {
  __shared__ unsigned wsum[PB / 64];
  const unsigned pini = scan[PH_PINI], num = scan[PH_NUM], base = scan[PH_BASE], total = scan[PH_TOTAL];
  if (!total || blockIdx.x * PB >= num) return;  // nothing listed (or it did not fit); uniform
  const unsigned i = blockIdx.x * PB + threadIdx.x;
  const unsigned p2 = pini + i;
  const unsigned f = (i < num) ? peri_flags(P, axis, a, p2) : 0u;
  const unsigned long long bp = __ballot(f & 1u), bm = __ballot(f & 2u);
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  const unsigned rank = unsigned(__popcll(bp & below) + __popcll(bm & below));  // entries of the lanes before
  if (lane == 0) wsum[wave] = unsigned(__popcll(bp) + __popcll(bm));
  __syncthreads();
  unsigned off = base + scan[PH_WORDS + blockIdx.x] + rank;
  for (unsigned w = 0; w < wave; w++) off += wsum[w];
  // (the scan admitted base + total <= cap; the guard keeps a disagreement out of memory)
  if ((f & 1u) && off < cap) peri_duplicate<WITHM1, WITHPRE>(P, K, axis, a, off, p2, false);
  off += (f & 1u);
  if ((f & 2u) && off < cap) peri_duplicate<WITHM1, WITHPRE>(P, K, axis, a, off, p2, true);
}

void launch_run_periodic(hipStream_t stm, unsigned cap, DevScalars* sc, const PeriConst& P, const KConst& K,
                         const PartArrays& a, bool withm1, bool withpre, unsigned* scan) {
  const unsigned nb = (cap + PB - 1) / PB;
  hipLaunchKernelGGL(k_peri_mark, dim3((cap + 255) / 256), dim3(256), 0, stm, sc, a.code, scan);
  for (int type = 0; type < 2; type++) {
    bool first = true;  // the type's first periodic axis: no new duplicates of it exist yet
    for (int axis = 0; axis < 3; axis++) {
      if (!(P.active & (1 << axis))) continue;
      // block 0 (the type's new duplicates so far) is empty on its first axis: not launched
      for (int block = first ? 1 : 0; block < 2; block++) {
        hipLaunchKernelGGL(k_peri_count, dim3(nb), dim3(PB), 0, stm, sc, P, a, scan, type, axis, block);
        hipLaunchKernelGGL(k_peri_scan, dim3(1), dim3(1024), 0, stm, sc, scan, type, block, cap);
        if (withm1 && withpre) hipLaunchKernelGGL((k_peri_write<true, true>), dim3(nb), dim3(PB), 0, stm, P, K, a, scan, axis, cap);
        else if (withm1) hipLaunchKernelGGL((k_peri_write<true, false>), dim3(nb), dim3(PB), 0, stm, P, K, a, scan, axis, cap);
        else if (withpre) hipLaunchKernelGGL((k_peri_write<false, true>), dim3(nb), dim3(PB), 0, stm, P, K, a, scan, axis, cap);
        else hipLaunchKernelGGL((k_peri_write<false, false>), dim3(nb), dim3(PB), 0, stm, P, K, a, scan, axis, cap);
      }
      first = false;
    }
  }
}

// ComputeAceMax with PeriActive (JSphCpuSingle.cpp:584-605): the normal particles of [npb, np).
__global__ __launch_bounds__(256) void k_peri_acemax(DevScalars* __restrict__ sc, const typecode* __restrict__ code,
                                                     const float4* __restrict__ arace) {
  const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
  float ace2 = 0.f;
  if (p >= sc->npb && p < sc->np && CodeIsNormal(code[p])) {
    const float4 ra = arace[p];
    ace2 = ra.x * ra.x + ra.y * ra.y + ra.z * ra.z;
  }
  block_max_atomic(sc, RED_ACEMAX2, ace2);
}

void launch_peri_acemax(hipStream_t stm, unsigned cap, DevScalars* sc, const typecode* code, const float4* arace) {
  hipLaunchKernelGGL(k_peri_acemax, dim3((cap + 255) / 256), dim3(256), 0, stm, sc, code, arace);
}

}  // namespace sphx
