// sph_gauge.hpp — the gauge system (JDsGaugeSystem / JDsGaugeItem) on the device.
//
// A gauge measures the fluid while the run goes on: velocity at a point (JGaugeVelocity), the
// free surface along a line (JGaugeSwl), the highest fluid particle near a vertical line
// (JGaugeMaxZ) or the pressure force on a boundary block (JGaugeForce).  Each has a compute
// schedule and an output schedule (JGaugeItem, JDsGaugeItem.h:103-111,164-165).  TimeStep lives
// on the device and steps are issued in batches, so the schedule decision, the evaluation and
// the record are made on the device, after the step's last update and before the motion and
// the divide (JSphCpuSingle.cpp:1094-1098): the kernels read the cell table of the last divide
// with the already-updated particles, as the reference does, and write nothing the solver reads.
//
// The schedule functions are plain inline functions (host and device) so that a CPU program
// can test them (tests/cpp/gauge_sched_host.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define SPH_GAUGE_HD __host__ __device__
#else
#define SPH_GAUGE_HD
#endif

namespace sphx {

// Compute and output timing of one gauge (JGaugeItem::ConfigComputeTiming / ConfigOutputTiming).
struct GaugeSched {
  double cstart, cend, cdt, cnext;  // ComputeStart, ComputeEnd, ComputeDt, ComputeNext
  double ostart, oend, odt, onext;  // OutputStart, OutputEnd, OutputDt, OutputNext
  int osave, pad;                   // OutputSave
};

// JGaugeItem::Update (JDsGaugeItem.h:164).
SPH_GAUGE_HD inline bool gauge_update(const GaugeSched& s, double t) {
  return t >= s.cnext && s.cstart <= t && t <= s.cend;
}
// JGaugeItem::Output (JDsGaugeItem.h:165).
SPH_GAUGE_HD inline bool gauge_output(const GaugeSched& s, double t) {
  return s.osave && t >= s.onext && s.ostart <= t && t <= s.oend;
}
// JGaugeItem::SetTimeStep (JDsGaugeItem.cpp:204-211): ComputeNext after a measure at t.
SPH_GAUGE_HD inline void gauge_set_timestep(GaugeSched& s, double t) {
  if (s.cdt) {
    const unsigned nt = unsigned(t / s.cdt);
    s.cnext = s.cdt * nt;
    if (s.cnext <= t) s.cnext = s.cdt * (nt + 1);
  }
}
// StoreResult's OutputNext (JDsGaugeItem.cpp:266-270), after a stored result at t.
SPH_GAUGE_HD inline void gauge_output_next(GaugeSched& s, double t) {
  if (s.odt) {
    const unsigned nt = unsigned(t / s.odt);
    s.onext = s.odt * nt;
    if (s.onext <= t) s.onext = s.odt * (nt + 1);
  }
}

enum { GAUGE_VEL = 0, GAUGE_SWL = 1, GAUGE_MAXZ = 2, GAUGE_FORCE = 3 };

// One gauge on the device.
struct GaugeDev {
  GaugeSched s;
  int type;
  unsigned pt0, npt;    // its sample points (one wave each): velocity 1, SWL PointNp+1, MaxZ 1, force 0
  unsigned pointnp;     // SWL: PointNp
  double p0[3];         // Point (velocity), Point0 (SWL, MaxZ)
  double dir[3];        // SWL: PointDir
  double height;        // MaxZ: Height
  float masslimit;      // SWL: MassLimit
  float distlimit;      // MaxZ: DistLimit
  unsigned code;        // force: CODE_GetTypeAndValue of the target block
  unsigned fslot;       // force: its slot of the per-block partial sums
  float res[3];         // result of the last measure
  unsigned pad;
};

// One sample point: its position (the SWL points by repeated addition of PointDir, as
// JGaugeSwl::CalculeCpuT walks them) and its gauge.
struct GaugePoint {
  double x, y, z;
  unsigned gauge, k;
};

// Record buffer state.
struct GaugeCtl {
  unsigned count;     // records held
  unsigned dropped;   // records dropped since the last drain (buffer full)
  unsigned pad[2];
};

}  // namespace sphx

// (a CPU test program of the schedule defines SPH_GAUGE_SCHED_ONLY: no HIP headers)
#ifndef SPH_GAUGE_SCHED_ONLY
#include "sph_kernels.hpp"

namespace sphx {

constexpr unsigned ERR_GAUGE_FULL = 64u;  // non-fatal: a gauge record found the buffer full and was dropped

struct GaugeSet {
  unsigned ng = 0, npts = 0, nforce = 0, nfblk = 0, reccap = 0;
  GaugeDev* gauges = nullptr;
  GaugePoint* pts = nullptr;
  double4* ptout = nullptr;     // [npts] per sample point: velocity sums / mass / zmax
  const unsigned* fidx = nullptr;  // [nforce] the force gauges
  double* fpart = nullptr;      // [nforce][nfblk][3] per-block sums of ace
  SphGaugeRecord* rec = nullptr;
  GaugeCtl* ctl = nullptr;
};

// Blocks of the force kernel (one lane per boundary particle) for a boundary capacity.
unsigned gauge_force_blocks(unsigned npbcap);
// Evaluates the gauges that are due at sc->time (all of them when `all`) into ptout / fpart.
void launch_gauge_eval(hipStream_t stm, const GaugeSet& gs, const DevScalars* sc, const PartArrays& a,
                       const unsigned* begincell, DivGrid g, const KConst& K, bool all);
// Finishes the due gauges' results; record = true: schedule update and records (a step);
// false: results only (sph_solver_measure).
void launch_gauge_commit(hipStream_t stm, const GaugeSet& gs, DevScalars* sc, const KConst& K, bool record);

}  // namespace sphx
#endif
