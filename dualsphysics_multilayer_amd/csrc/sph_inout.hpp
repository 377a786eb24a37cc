// sph_inout.hpp — inlet/outlet zones (sph_inout.hip): the zone data on the device and the
// launchers of the passes around the end-of-step divide.
#pragma once
#include "sph_kernels.hpp"

namespace sphx {

constexpr int INOUT_MAXZONES = 16;
// 16-bit typecode (DualSphDef.h:178-190, 218-223)
constexpr typecode CODE_MASKTYPEVALUE = 0x1fff, CODE_TYPE_FLUID_INOUT = 0x1fe0, CODE_TYPE_FLUID_INOUTNUM = 16,
                   CODE_TYPE_FLUID_INOUTMASK = 31, CODE_TYPE_FLUID_INOUT015MASK = 15;
__host__ __device__ inline bool CodeIsFluidInout(typecode c) { return (c & CODE_MASKTYPEVALUE) >= CODE_TYPE_FLUID_INOUT; }
__host__ __device__ inline bool CodeIsFluidNotInout(typecode c) {
  return CodeIsFluid(c) && (c & CODE_MASKTYPEVALUE) < CODE_TYPE_FLUID_INOUT;
}
// JSphInOutDef.h:42-83, JSphInOutZone.h:67-73
constexpr unsigned IO_VELP_MASK = 0x03, IO_VELP_LINEAR = 0x01, IO_VELP_PARABOLIC = 0x02;
constexpr unsigned IO_VELM_MASK = 0x0c, IO_VELM_FIXED = 0x00, IO_VELM_EXTRAPOLATED = 0x08;
constexpr unsigned IO_RHOP_MASK = 0x30, IO_RHOP_CONSTANT = 0x00, IO_RHOP_HYDROSTATIC = 0x10, IO_RHOP_EXTRAPOLATED = 0x20;
constexpr unsigned IO_CHECKINPUT = 0x80;
constexpr unsigned IO_REFILLADVANCED = 0x01, IO_REFILLSPFULL = 0x02, IO_REMOVEINPUT = 0x04, IO_REMOVEZSURF = 0x08,
                   IO_CONVERTINPUT = 0x10;

// One zone as the passes read it (JSphInOut's Planes, CfgZone, CfgUpdate, Width, DirData, VelData, Zsurf and
// the zone's BoxLimitMin/Max).
struct InOutZoneDev {
  float plane[4];
  float dir[3];
  float width;
  float vel0[4];  // the velocity profile's coefficients (VelData[2 i])
  float boxmin[3], boxmax[3];
  float zsurf;
  unsigned cfgzone, cfgupdate;
  unsigned pad;
};
// The inout data of a solver, in device memory (read by every inout kernel).
struct InOutDev {
  int nzones, useboxlimit, checkfreelimit, extrapmode;
  float freemin[3], freemax[3];
  float determlimit, coefhydro;
  unsigned codenewpart, pad;
  InOutZoneDev z[INOUT_MAXZONES];
};
// Scratch of the creation pass: scan words (block counts), the new zone of every particle.
size_t inout_scan_words(unsigned cap);
// InOutComputeStep before the end-of-step divide (JSphCpuSingle_InOut.cpp:146-210): the
// classification of the fluid in the checking zones, the zone rules and the new inlet particles
// appended behind np.  A pass whose new particles do not fit `cap` creates none and raises
// ERR_INOUT_FULL.  IdMax and the statistics live in DevScalars (io_*).
void launch_inout_step(hipStream_t stm, unsigned cap, DevScalars* sc, const InOutDev* io, const KConst& K,
                       const PartArrays& a, unsigned* scan, unsigned char* newiz);
// InOutUpdatePartsData after it (JSphCpuSingle_InOut.cpp:228-255): the analytical velocity and
// density, the extrapolation from the ghost nodes (list: scratch of cap entries), VelrhopM1, and
// what the divide derived from the velocities it sorted: press and VelMax.
void launch_inout_parts(hipStream_t stm, unsigned cap, DevScalars* sc, const InOutDev* io, const InOutDev& iohost,
                        const KConst& K, const DivGrid& g, const PartArrays& a, const unsigned* begincell, float* press,
                        unsigned* list, bool withm1);
// ComputeAceMax over the normal particles that are not inout (JSphCpuSingle.cpp:584-605).
void launch_inout_acemax(hipStream_t stm, unsigned cap, DevScalars* sc, const typecode* code, const float4* arace);

}  // namespace sphx
