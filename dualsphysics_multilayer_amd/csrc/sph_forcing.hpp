// sph_forcing.hpp — imposed accelerations (JDsAccInput) and damping zones (JDsDamping) on the
// device: the two per-particle passes of sph_forcing.hip and what the solver hands them.
#pragma once
#include "sph_kernels.hpp"

namespace sphx {

// ---- imposed accelerations (<special><accinputs>, JDsAccInput.cpp) ----
constexpr int ACC_MAXIN = 16;   // inputs (TypeAndValue ranges) of one solver
constexpr int ACC_ROWW = 13;    // doubles per table row: time, acc lin/ang [6], vel lin/ang [6]
struct AccInDev {               // JDsAccInputMk
  unsigned code1, code2;        // CodeSel1..CodeSel2 of CODE_GetTypeAndValue(code)
  int gravity;                  // GravityEnabled ("globalgravity": false subtracts Gravity)
  int first, n;                 // rows [first, first + n) of the table buffer
  int pad;
  double t0, t1;                // TimeIni, TimeEnd
  double centre[3];             // AccCoG (read as float, JDsAccInput.cpp:184)
};
struct AccInSet {               // by value to the kernels
  int n, pad;
  AccInDev in[ACC_MAXIN];
};
// The values of one input at the TimeStep of the interaction (StAceInput), written by
// k_accinput_eval; active = 0 outside [t0, t1] (codesel1 = UINT_MAX there).
struct AccVals {
  int active, withang;
  double acclin[3], accang[3], vellin[3], velang[3];
};
// JLinearValue's lookup state between calls (both tables of an input share their times).
struct AccState {
  int pos, posnext;
  double t;
};
// The values of every input at TimeStep (interstep 3: the step's start, sc->tstep0; else
// sc->time) into vals[], then arace.xyz += the imposed part over [npb, np) and AceMax over
// the same set into the (reset) RED_ACEMAX2 slots.
void launch_accinput(hipStream_t stm, unsigned cap, DevScalars* sc, const KConst& K, const DivGrid& g,
                     const AccInSet& set, const double* rows, AccState* state, AccVals* vals, int interstep,
                     const PartArrays& a, float4* arace);

// ---- damping zones (<special><damping>, JDsDamping.cpp) ----
constexpr int DAMP_MAXZONES = 16;
enum { DAMP_PLANE = 0, DAMP_BOX = 1, DAMP_CYL = 2 };
struct DampZoneDev {
  int type, usedomain, vertical, pad;
  float over, redumax, dist, pad2;  // OverLimit, ReduMax, Dist (plane, cylinder)
  float factor[3], pad3;            // Factorxyz
  double plane[4];                  // plane: Plane
  double zmin, zmax;                // plane domain
  double dompla[4][4];              // DomPla0..3
  double bmin1[3], bmin2[3], bmax1[3], bmax2[3], bover1[3], bover2[3], bsize1[3], bsize2[3];  // box
  double p1[3], p2[3];              // cylinder axis
  double rmin, axislen;             // LimitMin, PointsDist(Point1, Point2)
};
// Every zone in list order on the normal fluid particles' new velocity `velrhop`, with the
// step's dt (sc->dt).
void launch_damping(hipStream_t stm, unsigned cap, const DevScalars* sc, const KConst& K, const DivGrid& g,
                    const DampZoneDev* zones, int nzones, const PartArrays& a, float4* velrhop);

}  // namespace sphx
