// sph_solver_slab.cpp — SphGpuSingle as a slab of a decomposed domain: exchange, ghosts, face
// re-sends, re-partition; SphSlabGroup.
#include "sph_solver_impl.hpp"

#include <algorithm>
#include <chrono>
#include <exception>
#include <string>
#include <thread>
#include <vector>

namespace sphx {

// Slab exchange buffers sized once from the case, from its densest cell slice along the
// slab axis: W face slices of ghosts per face (+50 %), a quarter of that in migrants.  The face messages then
// need no hipMalloc (and no stream synchronisation) mid-run; the grow paths of Exchange()
// stay as the fallback for a flow that piles particles into a face column or a re-partition
// that hands over many columns at once.
void SphGpuSingle::PresizeExchange(const SphParticlesHost& h) {
  const int ax = slabcfg_.axis;
  std::vector<unsigned> cnt(size_t(C.dom_cells[ax]) + 1, 0u);
  unsigned mx = 0;
  for (unsigned p = 0; p < h.n; p++) {
    const double x = (h.pos[3 * p + ax] - C.dom_posmin[ax]) / double(C.scell);
    if (!(x >= 0.0)) continue;
    const size_t cx = size_t(x);
    if (cx < cnt.size()) mx = std::max(mx, ++cnt[cx]);
  }
  const unsigned long long g = (unsigned long long)mx * unsigned(ghost_width(C));
  sendg_.resize(slab_mincap_ ? 1 : g + g / 2 + 4096);
  sendm_.resize(slab_mincap_ ? 1 : g / 4 + 1024);
  BindSendBufs();
  recvg_.resize(2 * sendg_.cap());
  recvm_.resize(2 * sendm_.cap());
}

void SphGpuSingle::BindSendBufs() {
  send_.gcap = sendg_.cap();
  send_.gl = reinterpret_cast<SlabGhost*>(sendg_.ptr());
  send_.gr = send_.gl + send_.gcap;
  send_.mcap = sendm_.cap();
  send_.ml = reinterpret_cast<SlabRec*>(sendm_.ptr());
  send_.mr = send_.ml + send_.mcap;
}

// Slab exchange before the divide: pack the migrants and count the ghosts per face box
// (device), swap the face messages (migrant count, ghost count per face box) with both
// neighbours device to device, then ONE host wait to size the transfers; move the migrants
// (96-112 B records) and append them.  The divide reserves the ghosts' slots; their
// records follow it (launch_ghost_pack -> post; GhostCollect), beside the interaction of the
// items that need no ghost when the step allows it (OverlapGhosts).
void SphGpuSingle::Exchange() {
  const bool withm1 = (step_algorithm_ == SPH_STEP_VERLET), withpre = havepre_;
  const bool hl = transport_->has_left(), hr = transport_->has_right();
  if (!hl && !hr) return;  // a slab alone holds the whole domain: no ghosts, no migrants
  SLAB_TRACE("exchange: pack");
  // (the first pack's count pass may have run in the update kernel, FuseUpdate)
  auto pack = [&] {
    launch_slab_pack(stream, cap_, sc_, cur_, G, K, C.dom_posmin, hl, hr, withm1, withpre, packtiles_, slabcnt_,
                     send_, normal_, nnormal_, &faces_, packcounted_);
    packcounted_ = false;
  };
  // the pack rewrites the migrant and face-message send buffers: the neighbours' copies of
  // the last messages (in-process slabs copy asynchronously) are done first
  transport_->wait_sends(stream);
  // turns measurement mode 2: the pack kernels are a turn of their own
  const bool pturn = in_run_ && transport_->turns();
  if (pturn) transport_->turn_wait(SlabTransport::TURN_PACK, stream, nullptr);
  pack();  // (its accumulated counts were zeroed by the last exchange's kernels: no memset launches)
  if (pturn) transport_->turn_done(SlabTransport::TURN_PACK, stream);
  const size_t mb = 4 * (size_t(FMSG_HDR) + faces_.nfb);
  transport_->exchange(faces_.msg[0], hl ? mb : 0, faces_.msg[1], hr ? mb : 0, faces_.msg[2], hl ? mb : 0,
                       faces_.msg[3], hr ? mb : 0, stream);
  // received headers -> the counts the host reads; the prefixes of all four messages' counts
  // (slots of the received ghosts, records of the sent ones) in the same launch
  launch_face_scan(stream, faces_, slabcnt_, hl, hr);
  check_hip(hipMemcpyAsync(slabcnt_host_, slabcnt_, sizeof(SlabCounts), hipMemcpyDeviceToHost, stream),
            "exchange: read counts");
  // The transfer sizes must be on the host before the transfers are posted: the one host
  // wait of a divide.  Spin on an event (a blocking synchronise wakes up tens of us later);
  // the GPU idles from the counts copy until the next launches arrive.
  if (!xev_) check_hip(hipEventCreateWithFlags(&xev_, hipEventDisableTiming), "hipEventCreate");
  check_hip(hipEventRecord(xev_, stream), "exchange: event");
  WaitEvent(xev_, "exchange: wait counts");
  const SlabCounts c = *slabcnt_host_;
  SLAB_TRACE("exchange: counts");
  {
    // the neighbour's ghosts of this slab: the ghosts sent now + the migrants it sent here
    // (it keeps them as ghosts); the neighbour derives the same sizes from its counts.  They
    // size the face re-sends after the divide (NN eta / tau, SPS tau, mDBC densities) exactly
    face_sl_ = hl ? unsigned(c.sendl[0] + c.recvl[1]) : 0u;
    face_sr_ = hr ? unsigned(c.sendr[0] + c.recvr[1]) : 0u;
    face_rl_ = hl ? unsigned(c.recvl[0] + c.sendl[1]) : 0u;
    face_rr_ = hr ? unsigned(c.recvr[0] + c.sendr[1]) : 0u;
  }
  const unsigned long long gneed = std::max(c.sendl[0], c.sendr[0]), mneed = std::max(c.sendl[1], c.sendr[1]);
  if (gneed > sendg_.cap()) {  // the ghost records are packed after the divide: room for them
    transport_->drain_sends();  // the neighbours' reads of the old buffer are done
    check_hip(hipStreamSynchronize(stream), "exchange: sync");
    send_.gl = send_.gr = nullptr;  // (no capacity behind them until the new buffer is bound)
    send_.gcap = 0;
    sendg_.reserve(gneed, 4096, slab_mincap_);
    BindSendBufs();
  }
  if (mneed > sendm_.cap()) {  // migrant records past the capacity were not written: grow, pack again
    transport_->drain_sends();  // ... and the face messages are rewritten: their reads are done
    check_hip(hipStreamSynchronize(stream), "exchange: sync");
    send_.ml = send_.mr = nullptr;
    send_.mcap = 0;
    sendm_.reserve(mneed, 1024, slab_mincap_);
    BindSendBufs();
    // the counts accumulate again: start them over (the face messages already sent are unchanged)
    check_hip(hipMemsetAsync(&slabcnt_->nkeep, 0, sizeof(unsigned) * 3, stream), "exchange: reset nkeep, ghosts");
    for (int k = 0; k < 2; k++)
      check_hip(hipMemsetAsync(faces_.msg[k] + FMSG_HDR, 0, 4 * size_t(faces_.nfb), stream), "exchange: reset faces");
    pack();
  }
  const unsigned long long rgl = hl ? c.recvl[0] : 0, rgr = hr ? c.recvr[0] : 0;
  const unsigned long long rml = hl ? c.recvl[1] : 0, rmr = hr ? c.recvr[1] : 0;
  if (rgl + rgr > recvg_.cap()) {
    check_hip(hipStreamSynchronize(stream), "exchange: sync");
    recvg_.reserve(rgl + rgr, 4096, slab_mincap_);
  }
  if (rml + rmr > recvm_.cap()) {
    check_hip(hipStreamSynchronize(stream), "exchange: sync");
    recvm_.reserve(rml + rmr, 1024, slab_mincap_);
  }
  const unsigned long long nin = rgl + rgr + rml + rmr;  // the ghosts' slots are reserved by the divide
  if (c.np + nin > cap_) {
    const unsigned long long want = (c.np + nin) + (slab_mincap_ ? 16 : (c.np + nin) / 2);
    if (want >= (1ull << 31)) throw SphError(SPH_ERR_NOMEM, "slab particle capacity overflow");
    Grow(c.np, unsigned(want));
  }
  // k_unpack zeroes the face counts of the messages just sent: the neighbours have read them
  transport_->wait_sends(stream);
  // the migrants of both faces (two concurrent streams over the two xGMI links)
  transport_->exchange(send_.ml, sizeof(SlabRec) * c.sendl[1], send_.mr, sizeof(SlabRec) * c.sendr[1], recvm_.ptr(),
                       sizeof(SlabRec) * rml, recvm_.ptr() + rml, sizeof(SlabRec) * rmr, stream);
  launch_slab_unpack(stream, sc_, recvm_.ptr(), unsigned(rml + rmr), recvg_.ptr(), 0u, c.np, cur_, K, C.dom_posmin, withm1,
                     withpre, slabcnt_, normal_, nnormal_, &faces_, hl, hr);
  SLAB_TRACE("exchange: done");
  xg_sl_ = hl ? c.sendl[0] : 0;
  xg_sr_ = hr ? c.sendr[0] : 0;
  xg_rl_ = rgl;
  xg_rr_ = rgr;
  xg_nm_ = unsigned(rml + rmr);
  xg_np_ = unsigned(c.np + rml + rmr);
  inc_.nold = unsigned(c.np);  // the incremental divide places the appended [np, np + nm) apart
  inc_.napp = xg_nm_;
}

// The ghost records of the last divide: packed from the sorted face columns and posted by
// the divide (launch_ghost_pack -> SlabTransport::post), received from both neighbours on
// stream s, written into the slots the divide reserved.
void SphGpuSingle::GhostCollect(hipStream_t s) {
  SLAB_TRACE("ghosts: collect");
  transport_->collect(recvg_.ptr(), sizeof(SlabGhost) * xg_rl_, recvg_.ptr() + xg_rl_, sizeof(SlabGhost) * xg_rr_, s);
  launch_ghost_scatter(s, sc_, recvg_.ptr(), unsigned(xg_rl_ + xg_rr_), inc_.apppos + xg_nm_, cur_, K, C.dom_posmin,
                       poscell_, press_, G, inc_ok_ ? inc_.skeys : nullptr, nn_ ? phaseeos_ : nullptr);
}

// The ghosts of the last divide still in flight (end of a run): in place on the solver stream.
void SphGpuSingle::GhostFinish() {
  if (!ghost_pending_) return;
  if (ghost_split_) {  // packed and posted on the exchange stream
    GhostCollect(xstream_);
    check_hip(hipEventRecord(ev_ghost_, xstream_), "ghosts: event");
    check_hip(hipStreamWaitEvent(stream, ev_ghost_, 0), "ghosts: join");
  } else {
    GhostCollect(stream);
  }
  ghost_pending_ = false;
}

// The interaction of the items that reach no ghost column can run while the ghosts are in
// flight when nothing between the divide and it reads a ghost: the headline tiled kernel
// inside Run(), without mDBC (its correction reads ghosts first), bodies (their particle map
// is built after the divide) or the NN / Laminar+SPS / shifting kernels (face exchanges of
// per-particle values first).
bool SphGpuSingle::OverlapEligible() const {
  return slab() && in_run_ && tiled_ && !nn_ && !ext_ && !normal_ && !nftp_ && !nmotobj_ &&
         (transport_->has_left() || transport_->has_right());
}
bool SphGpuSingle::OverlapGhosts() const { return overlap_ && OverlapEligible(); }

// The one host wait of a slab divide: spin on the event (a blocking synchronise wakes up
// tens of us later) with a deadline, polling the transport's asynchronous error state.  A
// dead or failed peer ends this rank with SPH_ERR_COMM instead of a hang (the transport is
// aborted first, so the other ranks' pending transfers fail or time out too).
void SphGpuSingle::WaitEvent(hipEvent_t ev, const char* what) {
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spin = 0;; spin++) {
    const hipError_t q = hipEventQuery(ev);
    if (q == hipSuccess) return;
    if (q != hipErrorNotReady) check_hip(q, what);
    if ((spin & 1023u) == 1023u) {
      try {
        transport_->check_async();
      } catch (...) {
        transport_->abort();
        throw;
      }
      const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (sec > comm_timeout_s_) {
        transport_->abort();
        throw SphError(SPH_ERR_COMM, std::string(what) + ": no progress for " + std::to_string(int(sec)) +
                                         " s (a neighbour slab is gone or stalled)");
      }
    }
  }
}

// Periodic re-balancing of the x-slabs ("re-balanced every K steps"): the
// owned particles per global column (fluid + bound_weight x bound, the weights of
// sph_slab_partition) are summed over the ranks, every rank derives the same new column
// bounds from them, and the next exchange hands over whole columns as migrants.  Each
// bound stays strictly inside the two slabs it separates, so a particle moves at most
// one rank, and the copies a rank keeps of its outgoing migrants in its new ghost column
// (the usual pack rule) give the neighbours their ghost columns during the hand-over.
// Called between an update and the divide (all ranks, same step).
void SphGpuSingle::Repartition() {
  // (FuseUpdate leaves the count pass to the exchange at a re-partitioning divide)
  if (packcounted_) throw SphError(SPH_ERR_STATE, "internal: the update counted the pack of a re-partitioning divide");
  const int ncxg = int(C.dom_cells[slabcfg_.axis]), nr = slabcfg_.nranks;
  launch_column_counts(stream, cap_, sc_, cur_, G, K, ncxg, colcnt_);
  std::vector<float> bnd(size_t(nr) + 1, 0.f);
  bnd[size_t(slabcfg_.rank)] = float(slabcfg_.c0);  // each rank contributes its own bound
  if (slabcfg_.rank == nr - 1) bnd[size_t(nr)] = float(slabcfg_.c1);
  check_hip(hipMemcpyAsync(colcnt_ + 2 * ncxg, bnd.data(), 4 * bnd.size(), hipMemcpyHostToDevice, stream),
            "repartition: bounds");
  transport_->allreduce_sum_f32(colcnt_, 2 * ncxg + nr + 1, stream);
  std::vector<float> h(2 * size_t(ncxg) + size_t(nr) + 1);
  check_hip(hipMemcpyAsync(h.data(), colcnt_, 4 * h.size(), hipMemcpyDeviceToHost, stream), "repartition: read");
  if (!xev_) check_hip(hipEventCreateWithFlags(&xev_, hipEventDisableTiming), "hipEventCreate");
  check_hip(hipEventRecord(xev_, stream), "repartition: event");
  WaitEvent(xev_, "repartition: column counts");
  std::vector<int> old(size_t(nr) + 1);
  for (int r = 0; r <= nr; r++) old[size_t(r)] = int(h[2 * size_t(ncxg) + size_t(r)]);
  std::vector<double> w(static_cast<size_t>(ncxg));
  double total = 0;
  for (int c = 0; c < ncxg; c++) {
    w[size_t(c)] = double(h[size_t(c)]) + repart_bw_ * double(h[size_t(ncxg + c)]);
    total += w[size_t(c)];
  }
  std::vector<double> pre(size_t(ncxg) + 1, 0.0);
  for (int c = 0; c < ncxg; c++) pre[size_t(c) + 1] = pre[size_t(c)] + w[size_t(c)];
  double maxload = 0;
  for (int r = 0; r < nr; r++) maxload = std::max(maxload, pre[size_t(old[size_t(r) + 1])] - pre[size_t(old[size_t(r)])]);
  repart_last_imbalance_ = total > 0 ? maxload / (total / nr) : 1.0;
  if (!(repart_last_imbalance_ > 1.0 + repart_tol_)) return;
  std::vector<int> nb(old);
  const int W = min_slab_width(C);  // every slab keeps its two disjoint face column sets
  partition_from_prefix(pre, nr, nb.data(), W);
  for (int r = 1; r < nr; r++) {  // inside the two slabs it separates, and increasing
    nb[size_t(r)] = std::min(std::max(nb[size_t(r)], old[size_t(r) - 1] + W), old[size_t(r) + 1] - W);
    nb[size_t(r)] = std::max(nb[size_t(r)], nb[size_t(r) - 1] + W);
  }
  bool changed = false;
  for (int r = 1; r < nr; r++) {
    if (nb[size_t(r)] + W > nb[size_t(r) + 1]) return;  // the clamps left no valid split: keep the old one
    changed |= nb[size_t(r)] != old[size_t(r)];
  }
  if (!changed) return;
  slabcfg_.c0 = nb[size_t(slabcfg_.rank)];
  slabcfg_.c1 = nb[size_t(slabcfg_.rank) + 1];
  G = make_grid(C, &slabcfg_);
  keybits_ = bits_for(G.boxdiscard, 1);
  inc_valid_ = false;  // the box keys changed: the next divide sorts from scratch
  repart_count_++;
}

void SphGpuSingle::ShareDeviceCheck() {
  if (!slab() || transport_->nranks < 2) return;
  char bus[64] = {0};
  check_hip(hipDeviceGetPCIBusId(bus, int(sizeof(bus)) - 1, device), "hipDeviceGetPCIBusId");
  unsigned h = 2166136261u;  // FNV-1a of the bus id, kept below 2^23: exact as a float sum term
  for (const char* c = bus; *c; c++) h = (h ^ unsigned((unsigned char)*c)) * 16777619u;
  const float mine = float((h & 0x7fffffu) + 1u);
  const int nr = transport_->nranks;
  std::vector<float> v(size_t(nr), 0.f);
  v[size_t(slabcfg_.rank)] = mine;
  float* d = nullptr;
  check_hip(hipMalloc((void**)&d, sizeof(float) * size_t(nr)), "hipMalloc device check");
  check_hip(hipMemcpy(d, v.data(), sizeof(float) * v.size(), hipMemcpyHostToDevice), "device check");
  transport_->allreduce_sum_f32(d, nr, stream);
  check_hip(hipMemcpyAsync(v.data(), d, sizeof(float) * v.size(), hipMemcpyDeviceToHost, stream), "device check");
  check_hip(hipStreamSynchronize(stream), "device check");
  (void)hipFree(d);
  for (int r = 0; r < nr; r++)
    if (r != slabcfg_.rank && v[size_t(r)] == mine) MarkSharedDevice();
}

void SphGpuSingle::SetRepartition(unsigned every, double bound_weight, double tolerance) {
  if (!slab()) throw SphError(SPH_ERR_STATE, "re-partitioning applies to slab solvers only");
  if (!(bound_weight >= 0) || !(tolerance >= 0)) throw SphError(SPH_ERR_ARG, "invalid re-partition weights");
  repart_every_ = every;
  repart_bw_ = bound_weight;
  repart_tol_ = tolerance;
}

// The exchange stream and its events (created on first use).
void SphGpuSingle::ExchangeStream() {
  if (!xstream_) check_hip(hipStreamCreateWithFlags(&xstream_, hipStreamNonBlocking), "hipStreamCreate");
  if (!ev_div_) check_hip(hipEventCreateWithFlags(&ev_div_, hipEventDisableTiming), "hipEventCreate");
  if (!ev_ghost_) check_hip(hipEventCreateWithFlags(&ev_ghost_, hipEventDisableTiming), "hipEventCreate");
}

// Slabs, SPH velocity gradients: the owned face-column fluid particles' eta (and tau) to the
// neighbours, written into their ghost copies by idp before the second pass.  Fixed-size
// records (count in slot 0) sized from the last exchange, so no host wait.
void SphGpuSingle::NNFaceExchange() {
  // NN: the first pass's eta (+ ConstEq tau); single phase Laminar+SPS: the particles' SPS tau
  float* veta = sps_ ? nullptr : viscoeta_;
  float4* tau = sps_ ? cur_.tau : tau_;
  FaceExchange(
      nnface_,
      [&](NNFaceRec* sl, NNFaceRec* sr, unsigned nsl, unsigned nsr) {
        launch_nn_face_pack(stream, cap_, sc_, cur_, K, G, veta, tau, sl, sr, nsl, nsr, idxmap_, casenp_);
      },
      [&](NNFaceRec* rl, NNFaceRec* rr, unsigned nrl, unsigned nrr) {
        launch_nn_face_apply(stream, sc_, rl, rr, nrl, nrr, idxmap_, casenp_, cur_.idp, veta, tau, tau != nullptr);
      });
}

// Slabs, mDBC: the corrected densities of the owned face-column boundary (and floating)
// particles to the neighbours' ghost copies, by idp.
void SphGpuSingle::MdbcFaceExchange() {
  FaceExchange(
      mdbcface_,
      [&](MdbcFaceRec* sl, MdbcFaceRec* sr, unsigned nsl, unsigned nsr) {
        launch_mdbc_face_pack(stream, cap_, sc_, cur_, press_, K, G, sl, sr, nsl, nsr, bidx_, nnormal_, ftnormals_);
      },
      [&](MdbcFaceRec* rl, MdbcFaceRec* rr, unsigned nrl, unsigned nrr) {
        launch_mdbc_face_apply(stream, sc_, rl, rr, nrl, nrr, bidx_, nnormal_, cur_.idp, cur_.velrhop, press_);
      });
}

// A face re-send of per-particle values before an interaction.  Records per side = the face's
// particles at the last exchange + the count slot (slot 0): both sides of a face derive the
// same size, no face record can be dropped and no host wait is needed.  `buf` holds the
// send-left, send-right, receive-left, receive-right regions; pack(sl, sr, nsl, nsr) fills the
// first two and apply(rl, rr, nrl, nrr) reads the last two (null for a side without a
// neighbour: an end slab's grid keeps ghost columns on its outer side too).
template <class Rec, class Pack, class Apply>
void SphGpuSingle::FaceExchange(GrowBuf<Rec>& buf, Pack pack, Apply apply) {
  const bool hl = transport_->has_left(), hr = transport_->has_right();
  const unsigned nsl = hl ? face_sl_ + 1u : 0u, nsr = hr ? face_sr_ + 1u : 0u;
  const unsigned nrl = hl ? face_rl_ + 1u : 0u, nrr = hr ? face_rr_ + 1u : 0u;
  const unsigned long long need = 0ull + nsl + nsr + nrl + nrr;
  if (need > buf.cap()) {
    transport_->drain_sends();
    check_hip(hipStreamSynchronize(stream), "faces: sync");
    buf.reserve(need, 1024, slab_mincap_);
  }
  Rec *sl = buf.ptr(), *sr = sl + nsl, *rl = sr + nsr, *rr = rl + nrl;
  // the neighbours' copies of the last message out of these buffers are done before the
  // pack rewrites them (in-process slabs copy asynchronously)
  transport_->wait_sends(stream);
  pack(hl ? sl : nullptr, hr ? sr : nullptr, nsl, nsr);
  transport_->exchange(sl, sizeof(Rec) * nsl, sr, sizeof(Rec) * nsr, rl, sizeof(Rec) * nrl, rr, sizeof(Rec) * nrr,
                       stream);
  apply(hl ? rl : nullptr, hr ? rr : nullptr, nrl, nrr);
}

// The face sizes of the last exchange and the records the last mDBC face pack counted.
std::string SphGpuSingle::HaloDiag() {
  unsigned cnt[2] = {0u, 0u};
  if (mdbcface_.ptr() && slab()) {
    const bool hl = transport_->has_left(), hr = transport_->has_right();
    if (hl) check_hip(hipMemcpy(&cnt[0], &mdbcface_.ptr()[0].idp, 4, hipMemcpyDeviceToHost), "read face count");
    if (hr)
      check_hip(hipMemcpy(&cnt[1], &mdbcface_.ptr()[hl ? face_sl_ + 1u : 0u].idp, 4, hipMemcpyDeviceToHost),
                "read face count");
  }
  return "slab " + std::to_string(slabcfg_.rank) + " face sizes sl " + std::to_string(face_sl_) + " sr " +
         std::to_string(face_sr_) + " rl " + std::to_string(face_rl_) + " rr " + std::to_string(face_rr_) +
         ", mDBC records counted " + std::to_string(cnt[0]) + " / " + std::to_string(cnt[1]);
}

// ---- in-process slab group -----------------------------------------------------------
SphSlabGroup::SphSlabGroup(const SphCaseDef& cdef, const SphParticlesHost& all, int nslabs, const int* devices,
                           const int* bounds, int axis)
    : hub_(std::make_shared<LocalHub>(nslabs)) {
  if (nslabs < 1) throw SphError(SPH_ERR_ARG, "nslabs < 1");
  for (int i = 0; i < nslabs; i++) {
    SlabConfig sc;
    sc.rank = i;
    sc.nranks = nslabs;
    sc.c0 = bounds[i];
    sc.c1 = bounds[i + 1];
    sc.axis = axis;
    slabs.emplace_back(new SphGpuSingle(cdef, all, devices[i], sc, make_local_transport(hub_, i)));
  }
  // Slabs sharing a GPU: the ghosts go before the interaction (one item list).  There the
  // face launch of the overlap waits for the CU slots of the interior launch and of the
  // other slabs' work, and the in-process copies use the same GPU's engines: measured on the
  // cfg3 two-slab split, 13.72 ms/step without overlap vs 13.84-13.95 with it.
  // Slabs on their own GPUs keep the overlap (sph_slab_group_set_overlap changes either).
  for (int i = 0; i < nslabs; i++)
    for (int j = 0; j < nslabs; j++)
      if (i != j && devices[i] == devices[j]) slabs[i]->MarkSharedDevice();
  // one GPU: the dt maxima and the floating / re-partition sums reduce on the device
  hub_->onedev = std::all_of(devices, devices + nslabs, [&](int d) { return d == devices[0]; });
}

void SphSlabGroup::Run(unsigned nsteps) {
  const size_t n = slabs.size();
  std::vector<std::thread> th;
  std::vector<std::exception_ptr> err(n);
  std::vector<int> primary(n, 0);
  for (size_t i = 0; i < n; i++)
    th.emplace_back([&, i] {
      try {
        slabs[i]->Run(nsteps);
        slabs[i]->Sync();
        slabs[i]->CheckErrors();  // a fatal error halts every slab at the same step (DtVariable)
      } catch (const SphError& e) {
        err[i] = std::current_exception();
        primary[i] = std::string(e.what()).find("aborted by another slab") == std::string::npos;
        hub_->abort();
      } catch (...) {
        err[i] = std::current_exception();
        primary[i] = 1;
        hub_->abort();
      }
    });
  for (auto& t : th) t.join();
  for (size_t i = 0; i < n; i++)
    if (err[i] && primary[i]) {
      try {
        std::rethrow_exception(err[i]);
      } catch (const SphError& e) {
        // a face overflow is seen on every slab (folded): say where each slab stood
        if (std::string(e.what()).find("did not fit") == std::string::npos) throw;
        std::string m = e.what();
        for (size_t j = 0; j < n; j++) {
          try {
            m += "; " + slabs[j]->HaloDiag();
          } catch (...) {
          }
        }
        throw SphError(e.status, m);
      }
    }
  for (size_t i = 0; i < n; i++)
    if (err[i]) std::rethrow_exception(err[i]);
}

}  // namespace sphx
