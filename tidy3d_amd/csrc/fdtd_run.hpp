// The run loop of fdtd_run: a fragment of fdtd_capi.hip, included there once, inside its unnamed namespace, behind everything the
// methods call (FdtdSolver, the launchers, the pair plans).  Not a stand-alone header.
// One `Run` object per call: its members are the state of the run (what the locals of the former 800-line function held), its
// methods the schedules — each with the streams it issues on and the field sets it reads / writes in its header.  Conventions:
//   st = main stream, cs = comm stream (the second stream of the engine; an alias of st when the two were found not to overlap);
//   set A = h->f (current: E^n, H^{n-1/2}), set B = h->f2 (the other set of the ping-pong), set T = h->f3 (third set: the middle
//   step of shell / slab pairs, round-4 form); "swap" = swap_sets: B becomes current.
//   Cross-stream edges are hipEvents recorded on the producer and waited for on the consumer; nothing waits on the host inside
//   the loop except field-decay checks.  FDTD_OPT_DEBUG_SYNC = 1 puts a device-wide synchronisation behind every launch
//   (time_end) and every step: a schedule whose result then differs from the normal run has a missing edge
//   (tests/test_gpu_parity.py::test_schedules_do_not_depend_on_stream_timing).
//   The order of the correction launches around a single step's field update is defined in ONE place, h_side_terms / e_side_terms
//   (fdtd_capi.hip, beside the launchers): every single-step schedule here and in fdtd_run_bloch.hpp calls them.

// ---- what fdtd_run (Run) and fdtd_run_bloch (BlochRun, fdtd_run_bloch.hpp) share: free functions over one handle or the two of a
// Bloch pair (the first handle is the one whose events, communicator and shutoff settings count) ------------------------------------
using Handles = std::initializer_list<FdtdSolver*>;
// run entry: the last run's per-launch timing events go, no early stop yet, the run's clock starts on st
int run_begin(Handles hs, hipStream_t st) {
  for (FdtdSolver* h : hs) {
    for (hipEvent_t e : h->kev) hipEventDestroy(e);
    h->kev.clear(); h->kev_kind.clear();
    h->stats.stopped_early = 0;
  }
  FdtdSolver* h0 = *hs.begin();
  HIPCHK(h0, hipEventRecord(h0->ev0, st));
  return 0;
}
// a monitor records at step n
bool rec_at(const FdtdSolver* h, long long n) {
  for (const Monitor& m : h->mons) if (m.next < m.steps.size() && m.steps[m.next] == n) return true;
  return false;
}
// Tile-shape probing by default: when the default shape launches fewer workgroups than this.  The two runs differ ON RECORD, not
// by design: fdtd_run probes below two waves of workgroups at 4 waves per SIMD (256 CUs x 4 x 2), fdtd_run_bloch kept the earlier
// "one wave at 3" (256 x 3); and fdtd_run applies the size threshold (n_cells, autotune == 2) to a probe on request too, while
// fdtd_run_bloch applies it in front of both conditions.  Results do not depend on the shape.
constexpr long long kProbeBelowWgs = 2048, kProbeBelowWgsBloch = 768;
long long default_shape_wgs(const FdtdSolver* h) {
  return (long long)((h->g.nx + 255) / 256) * ((h->g.ny + h->rows_f - 1) / h->rows_f) * ((h->g.nz + h->zchunk_f - 1) / h->zchunk_f);
}
// the energy summed over the ranks of h's communicator (1 double every decay_every steps), on stream s — every RCCL call of a
// communicator is issued on ONE stream, in the same order on all ranks: the comm stream in fdtd_run, the step stream in fdtd_run_bloch
int allreduce_energy(FdtdSolver* h, double* en, hipStream_t s) {
  double* tmp = h->energy_dev;
  HIPCHK(h, hipMemcpyAsync(tmp, en, sizeof(double), hipMemcpyHostToDevice, s));
  NCCLCHK(h, ncclAllReduce(tmp, tmp, 1, ncclDouble, ncclSum, h->comm, s));
  HIPCHK(h, hipMemcpyAsync(en, tmp, sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  return 0;
}
// the verdict of a field-decay check on the summed energy `en`, written to every handle.  -> 1: the run ends here (diverged, the
// caller's progress callback asked for it, or the shutoff level is reached)
int decay_verdict(Handles hs, double en, FdtdProgressFn progress, void* user) {
  FdtdSolver* h0 = *hs.begin();
  if (!std::isfinite(en)) {
    for (FdtdSolver* h : hs) h->stats.diverged = 1;
    return 1;
  }
  if (en > h0->energy_max) for (FdtdSolver* h : hs) h->energy_max = en;
  const double decay = h0->energy_max > 0 ? en / h0->energy_max : 1.0;
  for (FdtdSolver* h : hs) h->stats.field_decay = decay;
  if (progress && progress(h0->step, 0.0, decay, user)) return 1;
  if (h0->shutoff > 0 && h0->step > h0->decay_ref && decay < h0->shutoff) {
    for (FdtdSolver* h : hs) h->stats.stopped_early = 1;
    return 1;
  }
  return 0;
}
// the end of a run: its time (ev0 -> ev1 of the first handle) and step count into every handle's stats, the per-kernel timers at zero
int run_stats(Handles hs) {
  FdtdSolver* h0 = *hs.begin();
  float ms = 0.f;
  HIPCHK(h0, hipEventElapsedTime(&ms, h0->ev0, h0->ev1));
  for (FdtdSolver* h : hs) {
    h->stats.run_ms = ms;
    h->stats.steps_done = h->step;
    h->stats.h_kernel_ms = h->stats.e_kernel_ms = h->stats.fused_kernel_ms = h->stats.shell_kernel_ms = h->stats.seam_kernel_ms = h->seam_flush_ms = 0.0;
    h->stats.h_kernel_launches = h->stats.e_kernel_launches = h->stats.fused_kernel_launches = h->stats.shell_kernel_launches = h->stats.seam_kernel_launches = 0;
  }
  return 0;
}

struct GraphRec { const float* set; int parity; hipGraphExec_t exec; };
// Axes whose CPML recursions a one-GPU sweep carries: by default all that have layers, FDTD_OPT_PML_FUSED = 0 keeps the slab kernels,
// any other mask selects axes; none when the workgroup with its halo wave would pass 512 threads (`fits` = false: the request alone,
// whatever the tile geometry — what Run::setup_schedules asks before the geometry is final)
int sweep_pml_axes(const FdtdSolver* h, bool fits = true) {
  if (!any_pml(h) || (fits && 64 * (h->rows_f + 1) > 512)) return 0;
  return (h->pml_fused < 0 ? 7 : h->pml_fused) & pml_in_sweep_mask(h);
}
// a CPML step as three launches by tile class (Run::fused_one): by default from 2^24 cells up
bool pml_three_launches(const FdtdSolver* h) { return h->pml_split < 0 ? n_cells(h) >= (1LL << 24) : h->pml_split != 0; }
// The form steps n and n + 1 take when they go out as one pair (Run::choose_pair decides, Run::loop dispatches):
//   Plain: one two-step sweep over the whole grid; Shell: the bulk as a two-step sweep, the CPML shell as two single steps (round-4 form);
//   Shell2: the shell as shell2_step_kernel boxes; Shell2Holes: the same with the planes of the source lists as z holes that take single
//   steps (a Shell2 plan may hold z holes too: the planes of dispersive cells its sweep does not advance — shell2_pair reads the plan).
enum class PairForm { None, Plain, Shell, Shell2, Shell2Holes };
struct PairChoice {
  PairForm form = PairForm::None;
  const ZPlan* zp = nullptr;           // Shell, Shell2, Shell2Holes: the bulk's plane intervals
  bool src_alive = false;              // the sweep's node table injects
  bool spg = false;                    // the pair carries paged source terms (Plain, Shell2)
  bool disp = false;                   // the pair advances the dispersive cells itself (Plain, Shell2)
};
// One launch group of a CPML step by tile class (Run::tile_split): planes [za, zc) lie between the z slabs, tile rows [ty_a, ty_c) of
// them between the y slabs; nby = all tile rows
struct TileSplit {
  int za, zc, ty_a, ty_c, nby;
  // planes in between: bottom and top tile rows [x y] / middle tile rows [x]
  FusedRange edge_rows(int pml_in) const { return {.k0 = za, .k1 = zc, .pml = pml_in & 3, .ty_n = ty_a + (nby - ty_c), .ty_a = ty_a, .ty_gap = ty_c - ty_a, .edge = true}; }
  FusedRange middle_rows(int pml_in) const { return {.k0 = za, .k1 = zc, .pml = pml_in & 1, .ty_n = ty_c - ty_a, .ty_a = 0, .ty_gap = ty_a}; }
};
// What differs between the two forms of a z-slab rank's step pair (Run::slab_pair)
struct SlabPair {
  ClipP clip;                          // the bulk's two-step sweep
  int pml; bool edge;                  // the hole steps: axes of in-sweep CPML, edge launch
  ShellSets s1, s2;                    // the hole steps' sets and parameter blocks: A -> T, T -> B
  bool psi; int psi_set[2];            // the two exchanges: H-side psi of the top plane travels, from which set
  bool shell2;                         // a rank that carries CPML: the shell's boxes around sgm go out, the psi sets swap, a shell2 pair is counted
};
struct Run {
  FdtdSolver* h;
  int64_t n_steps;
  FdtdProgressFn progress;
  void* user;
  // the run's configuration (setup)
  bool multi = false, nb_lo = false, nb_hi = false;
  int nz = 0;
  hipStream_t st = nullptr, cs = nullptr;
  bool fused_ok = false, fused = false, fused_multi = false;
  int b_lo = 0, b_hi = 0;              // fused z-slab schedule: boundary planes next to the lower / upper neighbour
  bool primed = false;                 // fused z-slab schedule: monitors pre-recorded, H-side pre-corrections applied, ghost planes in flight
  int pml_in_m = 0;                    // z-slab ranks: axes whose CPML recursions run inside the sweeps
  bool psi_ghosts = false;
  int tb_req = 0;
  bool tb_two_streams = false, tb_ok = false;
  std::vector<hipEvent_t> tb_ev;       // [2 s] = A(s) done, [2 s + 1] = B(s) done (two-stream mode)
  bool split_now = false, graph_ok = false;
  std::vector<GraphRec> graphs;
  bool f2_ok = false, f2s_ok = false, s2_ok = false, s2_deep = false, f2m_ok = false;
  bool s2_disp = false;                // shell2 pairs: every dispersive cell deep inside the bulk — its sweep advances them (no z holes)
  bool spg_ok = false;                 // lists the node table cannot hold go out as paged source terms while they inject (spg_setup)
  bool f2mc_ok = false, f2mc_deep = false;   // z-slab ranks with CPML: shell2 pairs with the planes next to a cut as z holes (sgm: their geometry)
  ShellGeom sg{}, sgm{};
  ZPlan zp_base, zp_src;               // the bulk's planes: without / with the z holes of the source lists
  ZPlan zp_s2, zp_s2h;                 // shell2 pairs: one interval [o0z, o1z) / the intervals between the z holes of the source lists (ok: usable)
  F2Plan f2_plan;
  int64_t done = 0;
  // the step being issued (begin_step)
  long long n = 0;
  bool rec = false;
  PairChoice pc;                       // steps n and n + 1 as one pair, and in which form (f2_plan: the monitors it records)

  // a debugging aid (FDTD_OPT_DEBUG_SYNC): everything issued so far has finished before anything else is issued
  void sync_point() { if (h->debug_sync) (void)hipDeviceSynchronize(); }
  bool decay_at(long long m) const { return h->decay_every > 0 && (m % h->decay_every) == 0; }
  // `count` steps from step n on may go out with nothing of the host's between them: that many are left, no decay check falls behind
  // any but the last (at n + 1 ... n + count - 1), and no monitor records at the steps named
  bool steps_free(long long n, int count, std::initializer_list<long long> no_rec = {}) const {
    if (done + count > n_steps) return false;
    for (int q = 1; q < count; ++q) if (decay_at(n + q)) return false;
    for (long long m : no_rec) if (rec_at(h, m)) return false;
    return true;
  }
  bool two_steps_free(long long n, std::initializer_list<long long> no_rec = {}) const { return steps_free(n, 2, no_rec); }
  // planes [za, zc) of [ki, ke) and tile rows [ty_a, ty_c) that no y / z slab of the in-sweep CPML touches (+ 1 plane below: the next
  // chunk's prologue must not see a slab).  fused_one passes ki = 0, ke = nz, where the clamps fall away: za = min(ke, max(ki, X)) with
  // 0 <= X <= nz is X, and zc = max(za, min(ke, Y)) is max(za, hi0) for Y = hi0 < nz and nz for Y = nz (za <= nz) — its former formula.
  TileSplit tile_split(int pml_in, int ki, int ke) const {
    const int R = h->rows_f, nby_all = (h->g.ny + R - 1) / R;
    const PmlAxisDev &py = h->pml[1], &pz = h->pml[2];
    const bool in_y = (pml_in & 2) && py.ns > 0, in_z = (pml_in & 4) && pz.ns > 0;
    const int za = std::min(ke, std::max(ki, (in_z && pz.lo > 0) ? std::min(nz, pz.lo + 1) : 0));
    const int zc = std::max(za, std::min(ke, (in_z && pz.hi0 < nz) ? pz.hi0 : nz));
    const int ty_a = (in_y && py.lo > 0) ? std::min(nby_all, py.lo / R + 1) : 0;
    const int ty_c = (in_y && py.hi0 < h->g.ny) ? std::max(ty_a, py.hi0 / R) : nby_all;
    return {za, zc, ty_a, ty_c, nby_all};
  }
  // fused z-slab schedule: the boundary chunks' thickness.  -> false: no room between a slab cut and the z-CPML
  bool boundary_chunks() {
    // boundary chunk: TWO planes per neighbour face (all the exchange needs, and it starts that much earlier).
    // Measured inside engines on the per-rank proxy, RCCL looped back (profiles/r03y_probe_boundary_chunk_thickness
    // .jsonl): 512 x 512 x 64 plain 0.186 ms per step at 16 planes, 0.175 at 8, 0.167 at 4, 0.163 at 2 and at 1; with
    // materials + CPML 0.319 -> 0.287; 128 planes 0.301 -> 0.297.  (Round 1's kernels preferred 16: r01h.)
    int zb = h->bnd_planes > 0 ? h->bnd_planes : std::min(kBndPlanes, nz / 4);
    zb = std::max(1, std::min(zb, nz / 2));
    b_lo = nb_lo ? zb : 0;
    b_hi = nb_hi ? zb : 0;
    // the z-CPML differentiates along z: its slabs must stay clear of the boundary chunks (whose
    // corrections run on the other stream and before the ghost planes of the new step arrive)
    const PmlAxisDev& pz = h->pml[2];
    if (nb_hi && pz.n_lo > 0) b_hi = std::min(b_hi, nz - pz.n_lo - 1);
    if (nb_lo && pz.n_hi > 0) b_lo = std::min(b_lo, nz - pz.n_hi - 1);
    return !((nb_hi && b_hi < 1) || (nb_lo && b_lo < 1));
  }
  // checks, streams, the variant (fused / two-pass, one GPU / z-slab rank), tile-shape and placement probes (both on st)
  int setup() {
    multi = h->comm != nullptr;     // also true for a 1-rank communicator (self exchange)
    nb_lo = h->cfg.bc[4] == FDTD_BC_NEIGHBOR, nb_hi = h->cfg.bc[5] == FDTD_BC_NEIGHBOR;
    if ((nb_lo || nb_hi) && !multi) return fail(h, "fdtd_run: neighbour faces need fdtd_comm_init");
    if (multi && refuse_lists_on_z_slabs(h, h, "fdtd_run")) return -1;      // (whole-grid lists: h_side_terms, fdtd_capi.hip)
    // (PMC on a plus face of a z-slab rank: x / y walls are local to every plane; a z wall belongs to the rank without an upper
    //  neighbour, whose interior launch must hold the wall's two image planes and the two they mirror)
    // (six planes: the boundary chunk next to the lower neighbour is one plane thick below eight planes, two from there on)
    if (multi && h->mirror_wall[2] >= 0 && (nb_hi || h->mirror_wall[2] != h->g.nz - 2 || h->g.nz < 6))
      return fail(h, "fdtd_run: a PMC plus face along z needs the last z-slab to hold the wall and at least 6 planes");
    nz = h->g.nz;
    // runs that use BOTH streams first make sure the two really overlap (once per engine; falls back to one stream)
    if ((multi || any_pml(h) || h->tblock > 4096) && probe_stream_overlap(h)) return -1;
    st = h->stream, cs = h->comm_stream;
    if (run_begin({h}, st)) return -1;
    if (multi && (nb_lo || nb_hi) && nz < 2) return fail(h, "fdtd_run: a z-slab needs at least 2 planes");
    // the fused sweep is the default single-GPU path whenever rows are float4-aligned
    // (a wide material table — more than 1023 media, 16-bit indices, no LDS copy: on one GPU the single-step sweep reads it on
    //  request, fused_step_kernel<., WIDE>; AUTO here is the two-pass kernels — the caller decides, tidy3d_amd/engine.py — and so is a z-slab rank)
    if (h->mat4b && multi && h->cfg.variant == FDTD_VARIANT_FUSED)
      return fail(h, "fdtd_run: more than %d media on a z-slab need the two-pass kernels (FDTD_VARIANT_ZMARCH / AUTO), not FDTD_VARIANT_FUSED", kMaxMedia - 1);
    fused_ok = (h->g.nx % 4 == 0) && h->rows_f <= 15 &&
               (h->cfg.variant == FDTD_VARIANT_FUSED || (h->cfg.variant == FDTD_VARIANT_AUTO && !h->mat4b));
    fused = !multi && fused_ok;
    // with a communicator every rank must take the same path: the fused z-slab schedule runs only on
    // explicit request (the host decides for all ranks, tidy3d_amd/engine.py), AUTO = two-pass
    if (multi && h->cfg.variant == FDTD_VARIANT_FUSED && !(fused_ok && nz >= 4))
      return fail(h, "fdtd_run: the fused z-slab schedule needs nx %% 4 == 0 and >= 4 planes per slab");
    fused_multi = multi && h->cfg.variant == FDTD_VARIANT_FUSED;
    // ---- pipelined fused z-slab schedule (fused_multi) -------------------------------------------
    // Per step, with  b_lo / b_hi  boundary planes next to a neighbour face:
    //   cs: sweep [0,b_lo) + [nz-b_hi,nz)  -> E-side corrections and next step's H-side pre-corrections
    //       of those planes -> ONE exchange (exchange_fused_all), which overlaps the interior sweep
    //   st: sweep [b_lo, nz-b_hi)          -> the same corrections of the interior planes
    // The next boundary sweep needs this exchange and the interior planes next to it (ev_e_int); the
    // next interior sweep needs only the boundary planes next to it (ev_e_bnd, recorded BEFORE the
    // exchange).  Invariant at the top of a step ("primed"): monitors pre-recorded, H-side
    // pre-corrections applied on all planes, ghost planes in flight on cs.  Steps that record
    // monitors, check the field decay or end the run use a joined tail on st instead and re-prime.
    b_lo = 0, b_hi = 0;
    if (fused_multi && !boundary_chunks())
      return fail(h, "fdtd_run: the fused z-slab schedule needs at least 2 planes between a slab cut and the z-PML");
    // Tile-shape probing: on request (FDTD_OPT_AUTOTUNE), and by default on one GPU when the default shape
    // launches less than one wave of workgroups (256 CUs x 3): there the z-chunk decides how much of the chip a
    // sweep fills (128^3: 344 workgroups at 16 planes per chunk, 0.045 ms per step; 688 at 8 planes, 0.034 ms —
    // profiles/r01m_narrow_grid_axis_shift.log) and the probe costs a dozen sweeps once.  Results do not depend
    // on the shape.  (autotune == 2 lifts the size threshold: test aid for the emulated library)
    bool under_one_wave = false;
    if (fused && !h->tuned && !h->user_geometry) under_one_wave = default_shape_wgs(h) < kProbeBelowWgs;
    if ((fused || fused_multi) && (h->autotune || under_one_wave) && !h->tuned && !h->user_geometry &&
        (n_cells(h) >= (1LL << 20) || h->autotune == 2)) {
      if (autotune_fused(h, st)) return -1;
      // the boundary-chunk thickness follows the chosen z-chunk (as before, the room is not checked again: the probe changes nothing
      // boundary_chunks reads, so what passed above passes here)
      if (fused_multi) (void)boundary_chunks();
    }
    // (a rank of a z-slab run samples its own slab; nothing is exchanged while it does.  >= 100: any size — test aid)
    if ((fused || fused_multi) && !h->placement_done && (h->placement_tries % 100) > 0 &&
        (n_cells(h) >= (fused ? (1LL << 24) : (1LL << 22)) || h->placement_tries >= 100)) {
      const int tries = h->placement_tries;
      h->placement_tries = tries % 100;
      const int prc = probe_placement(h, st);
      h->placement_tries = tries;
      if (prc) return -1;
    }
    primed = false;
    // z-slab ranks carry the CPML recursions inside their sweeps as one GPU does (same arithmetic and summation order):
    // the x / y recursions are local in z, the z recursion stays two planes clear of the cuts, and the one thing a rank
    // lacks — the H-side psi of its ghost plane -1, for the chunk prologue at plane 0 — comes with the ghost planes
    // (exchange_fused_all).  pml_in_m: axes inside the sweep; bits 0 / 1 agree on all ranks, bit 2 only end ranks have.
    // ON REQUEST only (FDTD_OPT_PML_FUSED > 0 on every rank): measured inside engines on the per-rank proxy (profiles/
    // r04p, r04q: 512 x 512 slabs with CPML on x and y, exchange included) the slab kernels win on thin slabs — 64 planes
    // 0.304 vs 0.352 ms, 128 planes 0.565 vs 0.594 — and tie at 256 (1.069 vs 1.067): the interior goes out as three
    // partial launches on one stream there, and the all-axes instantiation runs its few tiles at 2 waves per SIMD.
    pml_in_m = 0;
    if (fused_multi && any_pml(h) && h->pml_fused > 0 && 64 * (h->rows_f + 1) <= 512)
      pml_in_m = h->pml_fused & pml_in_sweep_mask(h);
    psi_ghosts = fused_multi && (pml_in_m & 3) != 0;
    return 0;
  }
  // z-slab ranks, planes [k0, k1): the E-side terms of step n (a plane range: no whole-grid lists — setup refuses them on z-slabs) ...
  void e_post(long long n, int k0, int k1, hipStream_t s, bool replica) { e_side_terms(h, n, k0, k1, s, false, 7 & ~pml_in_m, replica); }
  // ... and the H-side terms (E^n and H^{n-1/2} of these planes are complete: the images beyond PMC plus walls first)
  void h_pre(long long n, int k0, int k1, hipStream_t s, bool replica) {
    fill_mirror(h, s, k0, k1);
    h_side_terms(h, n, k0, k1, s, 7 & ~pml_in_m, replica);
  }
  // all planes on st: monitors of step n, H-side pre-corrections, then the exchange on cs
  int prime(long long n) {
    if (rec_at(h, n)) record_monitors(h, n, false, st);
    h_pre(n, 0, nz, st, false);
    advance_tfsf_aux(h, false, n, st, false);
    advance_tfsf_aux(h, false, n, st, true);
    HIPCHK(h, hipEventRecord(h->ev_e_int, st));
    HIPCHK(h, hipStreamWaitEvent(cs, h->ev_e_int, 0));
    HIPCHK(h, hipEventRecord(h->ev_e_bnd, cs));
    if (exchange_fused_all(h, cs, psi_ghosts)) return -1;
    primed = true;
    return 0;
  }
  // the schedules a run may use besides single steps: the fused z-slab pipeline, the slab-interleaved two-step schedule, captured step pairs
  int setup_schedules() {
    if (fused_multi) {
      // the comm-stream replica of the 1-D incident grids starts from the main one
      for (Tfsf& t : h->tfsf) {
        HIPCHK(h, hipMemcpyAsync(t.e1c, t.e1, ((size_t)t.n_aux + 1) * 4, hipMemcpyDeviceToDevice, st));
        HIPCHK(h, hipMemcpyAsync(t.h1c, t.h1, (size_t)t.n_aux * 4, hipMemcpyDeviceToDevice, st));
      }
      if (ensure_second_set(h)) return -1;
    }
    // Two-stream schedule of one step (st = main stream, cs = comm stream):
    //   cs: [H top plane] -> send/recv H -> [E bottom plane] -> send/recv E      (boundary planes first)
    //   st: [H interior ] ----------------> [E interior    ]
    // Cross-stream edges (RAW and WAR), one event each:
    //   ev_e_int : E interior of step n-1 done     -> cs may update/ship H top plane (reads E[nz-1])
    //   ev_e_bnd : E plane 0 of step n-1 done (cs) -> st may run H interior (reads E[0]) and monitors
    //   ev_h_int : H interior done                 -> cs may update E plane 0 (reads H[0])
    //   ev_h_bnd : H top plane done (cs)           -> st may run E interior (reads H[nz-1])
    // Ghost planes are only touched on cs, in stream order.  No host synchronisation in the loop.
    // ---- slab-interleaved two-step schedule (one GPU, fused sweep; FDTD_OPT_TBLOCK) ---------------------------------
    // Two time steps per pass over the grid, slab by slab of T planes:  A(s) = step n on slab s (set a -> set b),
    // B(s) = step n+1 on slab s (b -> a, IN PLACE of what A read), issued  A(0) A(1) B(0) A(2) B(1) ... : B(s) follows
    // A(s+1) because its top plane differentiates E^{n+1} of slab s+1's first plane, and it must not overwrite a's slab s
    // before A(s+1)'s chunk prologue has read its top plane.  What B(s) reads was written two launches earlier — 2 T planes
    // x 6 arrays, within the 256 MiB Infinity Cache for T <= 16 at 512^2 cells per plane — so per step pair the arrays
    // cross the HBM interface about three times (read a, write b, write a) instead of four.  Every correction launch takes
    // a plane range already (the z-slab schedule uses them the same way): H-side pre-corrections of a slab go out in front
    // of its sweep, E-side ones behind it.  The same kernels, the same arithmetic on the same values: bit-identical to
    // single steps (tests/test_emu_fused.py, tests/test_gpu_production_path.py).  Not with CPML or TFSF (their state is
    // advanced per whole step), not across a periodic z (the ghost planes wrap around the slab order), and only for step
    // pairs in which no monitor records and no field-decay check falls on the middle step.
    tb_req = h->tblock < 0 ? 0 : (h->tblock % 4096);
    tb_two_streams = h->tblock > 4096 && h->stream_overlap == 1;
    // (tb_pair's slabs are plane ranges: no whole-grid lists, h_side_terms in fdtd_capi.hip; no CPML: launch_pml launches nothing here)
    tb_ok = fused && tb_req > 0 && !any_pml(h) && h->tfsf.empty() && h->cfg.bc[4] != FDTD_BC_PERIODIC &&
                       h->mirror_wall[0] < 0 && h->mirror_wall[1] < 0 && h->mirror_wall[2] < 0 && !has_lists(h) && nz >= 2 * tb_req;
    h->two_step_pairs = 0;
    h->tblock_used = tb_ok ? tb_req : 0;
    // ---- captured step pairs (hipGraph) ------------------------------------------------------------------------------
    // Small grids are bound by dependent launches (64^3: three launches, 31 us per step; profiles/r02h): a run of steps
    // without monitor records or decay checks is captured ONCE as a graph of two steps (set a -> b -> a, psi parity back)
    // and replayed.  A graph bakes its kernel arguments, so the source kernels of a captured launch read the step counter
    // from device memory (step_dev + offset; the graph's last node advances it by two).  Same launches, same order, same
    // arguments otherwise: bit-identical to direct launches (tests/test_gpu_production_path.py).  One stream only: not
    // with the three-launch CPML split of large grids, not on z-slabs, not with per-launch timing events.
    split_now = pml_three_launches(h) && (sweep_pml_axes(h, false) & 6) != 0;
    graph_ok = fused && !tb_ok && !split_now && !(h->cfg.flags & FDTD_FLAG_TIME_KERNELS) && !has_lists(h) &&    // (first_list_kind says why)
                    h->use_graph > 0;      // on request only: measured on ROCm 7.2 (profiles/r3i) a replayed pair is ~3 us per step
                                           // SLOWER than launching its kernels (64^3 17.6 -> 20.8, 128^3 28.8 -> 31.4, 200^3 81.5 -> 84.0)
    h->graph_pairs = 0;
    return 0;
  }
  int tb_pair(long long n) {
    const int T = tb_req, S = (nz + T - 1) / T;
    if (ensure_second_set(h)) return -1;
    if (tb_two_streams && tb_ev.empty()) {
      tb_ev.resize((size_t)2 * S);
      for (hipEvent_t& e : tb_ev) HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    auto zs = [&](int s) { return std::min(nz, s * T); };
    auto stage_a = [&](int s) -> int {                     // h->f = a
      hipStream_t q = st;
      if (tb_two_streams && s >= 3) HIPCHK(h, hipStreamWaitEvent(q, tb_ev[(size_t)2 * (s - 3) + 1], 0));   // stay <= 3 slabs ahead of B
      const int k0 = zs(s), k1 = zs(s + 1);
      h_side_terms(h, n, k0, k1, q);
      if (launch_fused_range(h, q, {.k0 = k0, .k1 = k1})) return -1;
      swap_sets(h);                                        // h->f = b: the E-side corrections of step n act on E^{n+1}
      e_side_terms(h, n, k0, k1, q, false);
      swap_sets(h);
      if (tb_two_streams) HIPCHK(h, hipEventRecord(tb_ev[(size_t)2 * s], q));
      return 0;
    };
    auto stage_b = [&](int s) -> int {
      hipStream_t q = tb_two_streams ? cs : st;
      if (tb_two_streams) HIPCHK(h, hipStreamWaitEvent(q, tb_ev[(size_t)2 * std::min(s + 1, S - 1)], 0));
      const int k0 = zs(s), k1 = zs(s + 1);
      swap_sets(h);                                        // h->f = b (E^{n+1}, H^{n+1/2}), h->f2 = a
      h_side_terms(h, n + 1, k0, k1, q);
      const int rc = launch_fused_range(h, q, {.k0 = k0, .k1 = k1});
      swap_sets(h);                                        // h->f = a again: slab s now holds E^{n+2}, H^{n+3/2}
      if (rc) return -1;
      e_side_terms(h, n + 1, k0, k1, q, false);
      if (tb_two_streams) HIPCHK(h, hipEventRecord(tb_ev[(size_t)2 * s + 1], q));
      return 0;
    };
    if (stage_a(0)) return -1;
    for (int s = 1; s < S; ++s) {
      if (stage_a(s)) return -1;
      if (stage_b(s - 1)) return -1;
    }
    if (stage_b(S - 1)) return -1;
    if (tb_two_streams) HIPCHK(h, hipStreamWaitEvent(st, tb_ev[(size_t)2 * (S - 1) + 1], 0));
    h->two_step_pairs++;
    return 0;
  }
  // one step of the one-GPU fused path (n = its time step; rec_post: monitors record behind the sweep)
  int fused_one(long long n, bool rec_post) {
    // H-side corrections are additive: pre-apply them to H^{n-1/2}; E-side ones follow the sweep.
    // With pml_in the CPML recursions run inside the sweep (same arithmetic, no slab kernels).
    // pml_in = axes whose recursions run inside the sweep (sweep_pml_axes).  Inside the sweep the field values a slab
    // kernel would re-read and re-write stay in registers: only psi moves (32 B per cell and axis membership).
    const int pml_in = sweep_pml_axes(h);
    // (periodic z: the wrapped copies in the ghost planes were taken at the end of the last step, in front of this refresh —
    //  their images beyond an x / y wall are refreshed with the planes they copy; a z-slab rank receives its ghost planes
    //  refreshed by their owner)
    fill_mirror(h, st, h->cfg.bc[4] == FDTD_BC_PERIODIC ? -1 : 0, h->cfg.bc[4] == FDTD_BC_PERIODIC ? nz + 1 : nz);
    aniso_save(h, st);                     // (E^n of the nodes around fully anisotropic cells: the sweep's read set is this set)
    modulation_save(h, st);                // (E^n of the nodes inside time-modulated media)
    nonlinear_save(h, st);                 // (E^n and I^n of the nodes inside Kerr media)
    h_side_terms(h, n, 0, nz, st, 7 & ~pml_in);
    advance_tfsf_aux(h, false, n, st);
    if (h->cfg.bc[4] == FDTD_BC_PERIODIC) fill_ghost_h(h, st);   // ghost(-1) must carry the pre-corrections too
    // small grids are bound by dependent launches, not by occupancy: one launch of the all-axes instantiation
    if ((pml_in & 6) == 0 || !pml_three_launches(h)) {
      if (launch_fused(h, st, pml_in)) return -1;
    } else {
      // The instantiation that carries the y / z recursions holds their psi values in registers from the
      // top of a plane (occupancy 2-3); the one most tiles need carries x only.  Three launches over
      // disjoint tiles, the two small ones on the second stream, concurrent with the big one:
      //   (1) planes of the z slabs (+1 plane: the next chunk's prologue must not see a slab), all rows   [x y z]
      //   (2) planes in between: bottom and top tile rows (a row or the halo row in a y slab)              [x y]
      //   (3) planes in between, middle tile rows                                                         [x]
      const TileSplit t = tile_split(pml_in, 0, nz);
      HIPCHK(h, hipEventRecord(h->ev_h_int, st));
      HIPCHK(h, hipStreamWaitEvent(cs, h->ev_h_int, 0));
      if (launch_fused_range(h, cs, {.k0 = 0, .k1 = t.za, .pml = pml_in, .k2_0 = t.zc, .k2_1 = nz, .edge = true})) return -1;
      if (launch_fused_range(h, cs, t.edge_rows(pml_in))) return -1;
      HIPCHK(h, hipEventRecord(h->ev_h_bnd, cs));
      if (launch_fused_range(h, st, t.middle_rows(pml_in))) return -1;
      HIPCHK(h, hipStreamWaitEvent(st, h->ev_h_bnd, 0));
      swap_sets(h);
      swap_psi_h(h, pml_in);
    }
    if (rec_post) record_monitors(h, n, true, st);
    e_side_terms(h, n, 0, nz, st, true, 7 & ~pml_in);
    advance_tfsf_aux(h, true, n, st);
    fill_ghost_fused(h, st);
    return 0;
  }
  bool sources_alive(long long n) {
    for (const PointSrc& s : h->psrc) if (n >= s.n_steps) return false;
    for (const Tfsf& t : h->tfsf) if (n >= t.n_steps) return false;
    return true;
  }
  // 0 = the pair (n, n + 1) was replayed; 1 = capture not available (caller launches directly); < 0 = error
  int graph_pair(long long n) {
    hipGraphExec_t exec = nullptr;
    for (const GraphRec& r : graphs) if (r.set == h->f.ex && r.parity == (h->pml_parity | (h->pml_e_parity << 1))) exec = r.exec;
    if (!exec) {
      // everything a captured launch may allocate or upload must exist before the capture starts
      if (ensure_second_set(h)) return -1;
      if (const int pml_in = sweep_pml_axes(h); pml_in && ensure_pml_blocks(h, pml_in)) return -1;
      if (!h->step_dev && dev_alloc(h, &h->step_dev, 1)) return -1;
      const float* set0 = h->f.ex;
      const int par0 = h->pml_parity | (h->pml_e_parity << 1);
      const hipError_t eb = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
      if (eb != hipSuccess) { (void)hipGetLastError(); graph_ok = false; h->graph_status = -(100 + (int)eb % 100); return 1; }
      h->step_dev_mode = true;
      int rc = 0;
      for (int q = 0; q < 2 && !rc; ++q) { h->step_dev_off = q; rc = fused_one(n + q, false); }
      h->step_dev_mode = false;
      if (!rc) hipLaunchKernelGGL(step_counter_kernel, dim3(1), dim3(1), 0, st, h->step_dev, 2LL, 1);
      hipGraph_t graph = nullptr;
      const hipError_t ee = hipStreamEndCapture(st, &graph);
      if (rc) { if (graph) hipGraphDestroy(graph); return -1; }
      hipError_t ei = hipSuccess;
      if (ee != hipSuccess || !graph || (ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0)) != hipSuccess) {
        h->graph_status = ee != hipSuccess ? -(200 + (int)ee % 100) : -(300 + (int)ei % 100);
        (void)hipGetLastError();
        if (graph) hipGraphDestroy(graph);
        graph_ok = false;
        return h->f.ex == set0 && (h->pml_parity | (h->pml_e_parity << 1)) == par0 ? 1 : fail(h, "fdtd_run: graph capture failed half way");
      }
      hipGraphDestroy(graph);
      graphs.push_back({set0, par0, exec});
      h->graph_status = 1;
    }
    if (h->step_dev_value != n) hipLaunchKernelGGL(step_counter_kernel, dim3(1), dim3(1), 0, st, h->step_dev, n, 0);
    if (hipGraphLaunch(exec, st) != hipSuccess) return fail(h, "hipGraphLaunch failed: %s", hipGetErrorString(hipGetLastError()));
    h->step_dev_value = n + 2;
    h->graph_pairs++;
    return 0;
  }
  // a pair form that needs more memory than there is: the run keeps single steps instead of failing
  void give_up_for_memory(bool& ok) {
    (void)hipGetLastError();
    h->err.clear();
    ok = false;
    h->f2_off_reason = FDTD_F2_OFF_MEMORY;
  }
  // which forms of step pairs this run may take (decided once; begin_step judges every pair): plain pairs, shell pairs (round-4
  // form), shell2 pairs, slab pairs of a z-slab rank — and what they need (source tables, the third field set, two streams)
  int setup_pairs() {
    // dispersive cells inside the two-step sweeps (round 6): their pole states move into paged storage, once
    if (fused && !tb_ok && !h->ade.empty() && disp_setup(h)) return -1;
    h->disp.pairs = 0;
    s2_disp = false;
    // paged source terms (round 6): a TFSF box, a mode plane, a current sheet, any list of more than kMaxInj nodes
    spg_ok = false;
    h->spg.pairs = 0;
    if (fused && !tb_ok && !multi && !h->mat4b && (!h->tfsf.empty() || !h->psrc.empty())) {      // (a wide table: no pairs, nothing to page)
      if (fused2_sources(h)) return -1;            // (src_nodes, the seam flags)
      bool needs = !h->tfsf.empty() || h->src_nodes > kMaxInj || h->src_h_on_seam || (h->src_h_nodes > 0 && !h->src_tab);
      if (!needs) {                                // lists of different lengths: mixed alive / spent pairs
        long long len = -1;
        for (const PointSrc& s : h->psrc) if (s.has_nodes()) { if (len >= 0 && s.n_steps != len) needs = true; len = s.n_steps; }
      }
      if (h->spg.state != 0 && (h->spg.n_psrc != h->psrc.size() || h->spg.n_tfsf != h->tfsf.size())) spg_release(h);      // (lists added since)
      if (needs && spg_setup(h)) return -1;
      // (absorber layers damp H^{n-1/2} inside the sweep, behind the H-side terms of step n that precede it: FDTD_F2_OFF_H_SOURCE_ABSORBER stays)
      spg_ok = needs && h->spg_on != 0 && h->spg.state == 1 && !(h->has_damp && h->spg.any_h);
    }
    f2_ok = fused && !tb_ok && fused2_eligible(h);
    sg = ShellGeom{};
    f2s_ok = false;
    h->f2_off_reason = !fused ? FDTD_F2_OFF_VARIANT : (tb_ok ? FDTD_F2_OFF_DISABLED : 0);
    if (fused && !tb_ok && !f2_ok) {
      const bool shell = any_pml(h) || any_periodic(h) || !h->ade.empty();
      h->f2_off_reason = shell ? shell_why_not(h, &sg, &zp_base, &zp_src) : fused2_why_not(h);
      f2s_ok = shell && h->f2_off_reason == 0;
    }
    // shell2 pairs: the shell by shell2_step_kernel (two steps per sweep, psi carried) instead of two single steps
    s2_ok = false, s2_deep = false;
    if (fused && !tb_ok && !f2_ok && any_pml(h)) {
      ShellGeom g2{};
      const int why2 = shell2_why_not(h, &g2);
      if (why2 == 0) {
        const int why_r4 = h->f2_off_reason;
        s2_ok = true; sg = g2;                               // (the same geometry shell_why_not finds)
        s2_deep = shell2_sources_deep(h, sg);
        h->f2_off_reason = 0;
        // the bulk's planes: one interval, or — dispersive cells — the intervals between their planes (z holes, inside the bulk's range)
        zp_s2 = ZPlan{};
        // (round 6: the pair advances the dispersive cells itself — the bulk sweep and the shell's boxes subtract their paged memory
        //  terms, ade2_kernel follows; not beside the single steps of a periodic y's wrap rows, not with the measuring-aid box cuts)
        s2_disp = !h->ade.empty() && h->disp.state == 1 && h->cfg.bc[2] != FDTD_BC_PERIODIC && h->shell2_on != 2 && h->shell2_on != 3;
        if (h->ade.empty() || s2_disp) { zp_s2.n = 1; zp_s2.a[0] = sg.o0[2]; zp_s2.b[0] = sg.o1[2]; zp_s2.ok = true; }
        else if (zplan_build(h, sg, false, &zp_s2) && zp_s2.a[0] == sg.o0[2] && zp_s2.b[zp_s2.n - 1] == sg.o1[2]) zp_s2.ok = true;
        if (!zp_s2.ok) { s2_ok = false; s2_disp = false; h->f2_off_reason = why_r4; }       // (the round-4 form may still take the run)
        // lists that inject and that the sweeps cannot apply: their planes as z holes — usable when every hole lies inside the bulk's plane
        // range (one-launch form only: FDTD_OPT_SHELL2 = 2 / 3 cut their boxes differently)
        zp_s2h = ZPlan{};
        if (h->shell2_on != 2 && h->shell2_on != 3 && zplan_build(h, sg, true, &zp_s2h) && zp_s2h.n > 1 && zp_s2h.a[0] == sg.o0[2] &&
            zp_s2h.b[zp_s2h.n - 1] == sg.o1[2]) zp_s2h.ok = true;
      }
    }
    h->f2_dyn_reason = 0;
    if (f2_ok || f2s_ok || s2_ok) {
      if (fused2_sources(h)) return -1;
    }
    // (the third field set: + 50 % field memory.  Where it does not fit, the run keeps single steps instead of failing)
    if (f2s_ok && ensure_third_set(h)) give_up_for_memory(f2s_ok);
    if ((f2s_ok || s2_ok) && probe_stream_overlap(h)) return -1;
    // z-slab ranks (pipelined schedule): step pairs with the planes next to the neighbour faces as the shell
    f2m_ok = fused_multi && !any_pml(h) && !h->has_damp && h->shell_on != 0 && nz >= 8 && fused2_why_not(h, true) == 0;
    if (fused_multi) h->f2_off_reason = f2m_ok ? 0 : (any_pml(h) || h->has_damp ? FDTD_F2_OFF_COMM : (fused2_why_not(h, true) ? fused2_why_not(h, true) : FDTD_F2_OFF_COMM));
    if (f2m_ok) {
      if (fused2_sources(h)) return -1;
      if (ensure_third_set(h)) give_up_for_memory(f2m_ok);
    }
    // z-slab ranks that carry CPML inside their sweeps (FDTD_OPT_PML_FUSED on every rank: tidy3d_amd/dist.py asks for it where the
    // whole problem allows it): shell2 pairs — bulk and boxes as on one GPU, over the planes two or more away from a cut; the two
    // planes next to a cut take two single steps as a z hole and ship their planes after each (slab_pair)
    f2mc_ok = false;
    if (fused_multi && any_pml(h) && pml_in_m != 0 && pml_in_m == pml_in_sweep_mask(h) && !h->has_damp && h->shell_on != 0 &&
        h->shell2_on != 0 && h->shell2_on != 2 && h->shell2_on != 3 &&      // (2 / 3: boxes cut by axes ignore the z range the cut planes' hole leaves them)
        h->ade.empty() && !any_periodic(h) && (long long)h->g.sxy * 4 < (1LL << 32)) {
      int why = fused2_why_not(h, true, true);
      if (!why && !shell_geometry(h, &sgm)) why = FDTD_F2_OFF_PML;
      if (!why) {
        const PmlAxisDev& pz = h->pml[2];
        if (nb_lo) sgm.o0[2] = std::max(sgm.o0[2], 2);
        if (nb_hi) sgm.o1[2] = std::min(sgm.o1[2], nz - 2);
        // (the z recursion stays clear of the holes' planes and of what their first step reads)
        if (sgm.o1[2] - sgm.o0[2] < 8 || (pz.ns > 0 && ((nb_lo && pz.lo > 0) || (nb_hi && pz.hi0 < nz)))) why = FDTD_F2_OFF_TOO_SMALL;
      }
      f2mc_ok = why == 0;
      h->f2_off_reason = why;
      if (f2mc_ok && (fused2_sources(h) || ensure_third_set(h) || ensure_pml_blocks2(h) || ensure_pml_blocks_hole(h))) give_up_for_memory(f2mc_ok);
      f2mc_deep = f2mc_ok && shell2_sources_deep(h, sgm);
    }
    h->fused2_pairs = 0;
    h->seam_deferred_pairs = h->seam_flushes = 0;
    h->shell_pairs = 0;
    h->shell2_pairs = 0;
    done = 0;
    return 0;
  }
  // the events between the bulk's stream and the shell's (created with the first shell pair of the handle)
  int shell_events() {
    if (h->ev_shell_a) return 0;
    HIPCHK(h, hipEventCreateWithFlags(&h->ev_shell_a, hipEventDisableTiming));
    HIPCHK(h, hipEventCreateWithFlags(&h->ev_shell_b, hipEventDisableTiming));
    return 0;
  }
  // the middle step of a shell pair on set T: E-side sources / TFSF corrections of step n, the dispersive cells' memory term, the incident
  // grid's E; then what precedes step n + 1: its H-side sources / corrections, the incident grid's H
  void middle_step(long long n, hipStream_t cs, const FieldP& T) {
    launch_sources(h, true, n, 0, nz, cs, false, &T);
    launch_ade(h, 0, nz, cs, &T);
    advance_tfsf_aux(h, true, n, cs);
    launch_sources(h, false, n + 1, 0, nz, cs, false, &T);
    advance_tfsf_aux(h, false, n + 1, cs);
  }
  // steps n and n + 1 of a grid walled by CPML: the bulk as ONE two-step sweep on st, the shell as two single steps on cs
  int shell_pair(long long n, const F2Table* tb, const ZPlan& zp) {
    hipStream_t cs = (h->shell_on == 2) ? st : h->comm_stream;       // (2: shell behind the bulk on ONE stream — a measuring aid)
    const int pml_in = 7 & pml_in_sweep_mask(h);
    if (ensure_second_set(h) || ensure_third_set(h) || ensure_pml_blocks(h, pml_in)) return -1;
    if (shell_events()) return -1;
    const int N[3] = {h->g.nx, h->g.ny, nz};
    int in0[3], in1[3];                                    // step one: the bulk shrunk by one cell (x: one lane) on its CPML sides
    for (int a = 0; a < 3; ++a) {
      in0[a] = sg.o0[a] > 0 ? sg.o0[a] + (a == 0 ? 4 : 1) : 0;
      in1[a] = sg.o1[a] < N[a] ? sg.o1[a] - (a == 0 ? 4 : 1) : N[a];
    }
    // (the order of a single step: H-side sources and TFSF corrections of step n on H^{n-1/2}, then the incident grid's H)
    launch_sources(h, false, n, 0, nz, st);
    advance_tfsf_aux(h, false, n, st);
    if (h->cfg.bc[4] == FDTD_BC_PERIODIC) fill_ghost_h(h, st);   // ghost(-1) must carry them too (as in a single step)
    HIPCHK(h, hipEventRecord(h->ev_shell_a, st));
    HIPCHK(h, hipStreamWaitEvent(cs, h->ev_shell_a, 0));
    const FieldP A = h->f, B = h->f2, T = h->f3;
    const int par = h->pml_parity;
    bool s2 = false;
    for (int i = 0; i < zp.n; ++i) {                       // the bulk: one clipped two-step sweep per interval of its planes
      const ClipP clip{sg.o0[0], sg.o1[0], sg.o0[1], sg.o1[1], zp.a[i], zp.b[i]};
      if (launch_fused2(h, n, st, tb, &s2, nullptr, &clip)) return -1;
    }
    if (launch_shell_step(h, A, T, par, in0, in1, pml_in, cs, zp, 1)) return -1;
    middle_step(n, cs, T);
    fill_ghost_fused(h, cs, &T);                           // periodic z: the middle step's wrapped planes (its top and bottom planes are the shell's)
    if (launch_shell_step(h, T, B, par ^ 1, sg.o0, sg.o1, pml_in, cs, zp, 0)) return -1;
    HIPCHK(h, hipEventRecord(h->ev_shell_b, cs));
    HIPCHK(h, hipStreamWaitEvent(st, h->ev_shell_b, 0));
    swap_sets(h);
    pair_record(h, tb, n, st);
    if (rec_at(h, n + 1)) record_monitors(h, n + 1, true, st);
    launch_sources(h, true, n + 1, 0, nz, st);
    launch_ade(h, 0, nz, st);
    advance_tfsf_aux(h, true, n + 1, st);
    fill_ghost_fused(h, st);
    return 0;
  }
  // steps n and n + 1 of a grid walled by CPML, shell2 form: the bulk as ONE clipped two-step sweep on st, the shell's boxes as
  // shell2_step_kernel launches on cs — all read set A / the current psi sets, all write disjoint cells of set B / the other psi sets
  // `zp`: the bulk's plane intervals.  One interval [o0z, o1z): no holes.  More: the planes between two intervals are z HOLES — the
  // planes of source lists the sweeps cannot apply while they inject (a mode plane, a current sheet, the injection plane of a plane
  // wave; +- 2 planes) — and take two single steps through set T on cs, as in the round-4 form, with parameter blocks that route
  // their psi through temporary sets (ensure_pml_blocks_hole); every interval gets its own bulk launch and its own boxes.
  int shell2_pair(long long n, const F2Table* tb, const ZPlan& zp) {
    hipStream_t cs = (h->shell_on == 2) ? st : h->comm_stream;       // (2: shell behind the bulk on ONE stream — a measuring aid)
    const bool holes = zp.n > 1;
    // a periodic y: the two rows on either side of the wrap belong to no box and to no bulk launch — they take two single steps
    // through set T beside them, over every plane outside the holes (whose steps cover all rows), with the holes' parameter blocks
    const bool per_y = h->cfg.bc[2] == FDTD_BC_PERIODIC;
    if (ensure_second_set(h) || ensure_pml_blocks2(h)) return -1;
    if ((holes || per_y) && (ensure_third_set(h) || ensure_pml_blocks_hole(h))) return -1;
    if (shell_events()) return -1;
    launch_sources(h, false, n, 0, nz, st);                  // H-side sources of step n on H^{n-1/2}, then the incident grid's H: the order of a single step
    if (pc.spg) spg_fill(h, n, st);                          // (paged source terms of the pair; the incident grids through both steps)
    else advance_tfsf_aux(h, false, n, st);
    const SrcP sr = pc.spg ? spg_params(h) : SrcP{};
    HIPCHK(h, hipEventRecord(h->ev_shell_a, st));
    HIPCHK(h, hipStreamWaitEvent(cs, h->ev_shell_a, 0));
    const FieldP A = h->f, B = h->f2, T = h->f3;
    const int hp = h->pml_parity, ep = h->pml_e_parity;
    bool s2 = false;
    Shell2Box boxes[kShell2MaxBoxes];
    int nb = 0;
    for (int i = 0; i < zp.n; ++i) {
      const ClipP clip{sg.o0[0], sg.o1[0], sg.o0[1], sg.o1[1], zp.a[i], zp.b[i]};
      // (one interval and every source node deep inside it: the sweep applies the E-side terms of step n + 1 itself)
      if (launch_fused2(h, n, st, tb, &s2, nullptr, &clip, pc.disp, zp.n == 1 && s2_deep, sr)) return -1;
      // the boxes beside this interval: its planes, and (first / last interval) the z slabs below / above
      ShellGeom gi = sg;
      gi.o0[2] = zp.a[i]; gi.o1[2] = zp.b[i];
      Shell2Box bi[kShell2MaxBoxes];
      const int ni = shell2_boxes(h, gi, bi, i == 0 ? 0 : zp.a[i], i == zp.n - 1 ? nz : zp.b[i]);
      for (int q = 0; q < ni && nb < kShell2MaxBoxes; ++q) boxes[nb++] = bi[q];
    }
    // dispersive cells (all deep inside the bulk): both steps of their pole states and the correction of E^{n+2} behind the bulk,
    // beside the shell's boxes, once nothing else is due on E^{n+2} there — else at the end, behind the sources of step n + 1
    const bool src_due = e_sources_due(h, n + 1);
    // (clear of the bulk's faces by what the boxes read beyond their own cells — a plane, two rows, a halo lane: ade2_kernel REWRITES the
    //  paged memory terms, and a box that has not yet read those of its halo plane would subtract the next pair's.  Found on the device by
    //  scripts/fuzz_round6.py in the round's last hour (seed 31, case 124: a Lorentz body whose lowest plane is the bulk's first one — one run
    //  in a few; the emulator, which runs the streams in issue order, shows it every time: tests/test_emu_disp.py).)
    const bool ade2_early = pc.disp && (s2 || !src_due) && disp_inside(h, sg.o0, sg.o1, 2);
    if (ade2_early) launch_ade2(h, st, &B);
    launch_shell2_boxes(h, boxes, nb, h->pml_blk2[hp][ep], cs, tb, pc.disp, sr);
    if (holes || per_y) {
      const int pml_in = 7 & pml_in_sweep_mask(h);
      ShellSets s1{A, T, hp, 0, 0, h->pml_blk_hole[0][hp][ep]}, s2h{T, B, hp, 0, 0, h->pml_blk_hole[1][hp][ep]};
      // the rows next to a periodic y wrap, grown by `grow` rows: the tile rows that hold them, the rows between left alone
      auto wrap_rows = [&](const ShellSets& base, int grow) {
        const int R = h->rows_f, ny = h->g.ny, nby_all = (ny + R - 1) / R;
        const int in0 = 2 + grow, in1 = ny - 2 - grow;
        const int ty_a = std::min(nby_all, (in0 + R - 1) / R), ty_c = std::max(ty_a, in1 / R);
        ShellSets sh = base;
        sh.ex_j0 = in0; sh.ex_j1 = in1;
        for (int i = 0; i < zp.n; ++i) {
          const int lo = i == 0 ? 0 : zp.a[i], hi = i == zp.n - 1 ? nz : zp.b[i];
          if (launch_fused_range(h, cs, {.k0 = lo, .k1 = hi, .pml = pml_in, .ty_n = ty_a + (nby_all - ty_c), .ty_a = ty_a, .ty_gap = ty_c - ty_a, .edge = true, .sh = &sh})) return -1;
        }
        return 0;
      };
      // step one over the holes grown by one plane (what step two differentiates), set A -> set T
      for (int i = 0; i + 1 < zp.n; ++i)
        if (launch_fused_range(h, cs, {.k0 = zp.b[i] - 1, .k1 = zp.a[i + 1] + 1, .pml = pml_in, .edge = true, .sh = &s1})) return -1;
      if (per_y && wrap_rows(s1, 1)) return -1;
      if (holes) middle_step(n, cs, T);
      for (int i = 0; i + 1 < zp.n; ++i)
        if (launch_fused_range(h, cs, {.k0 = zp.b[i], .k1 = zp.a[i + 1], .pml = pml_in, .edge = true, .sh = &s2h})) return -1;
      if (per_y && wrap_rows(s2h, 0)) return -1;
    }
    HIPCHK(h, hipEventRecord(h->ev_shell_b, cs));
    HIPCHK(h, hipStreamWaitEvent(st, h->ev_shell_b, 0));
    swap_sets(h);
    swap_psi_h(h, 7);
    swap_psi_e(h);
    pair_record(h, tb, n, st);
    if (rec_at(h, n + 1)) record_monitors(h, n + 1, true, st);
    if (!holes && !pc.spg) {
      advance_tfsf_aux(h, true, n, st);
      advance_tfsf_aux(h, false, n + 1, st);
    }
    if (!s2) launch_sources(h, true, n + 1, 0, nz, st);
    if (!pc.disp) launch_ade(h, 0, nz, st);
    else if (!ade2_early) launch_ade2(h, st);
    if (!pc.spg) advance_tfsf_aux(h, true, n + 1, st);
    fill_ghost_fused(h, st);
    return 0;
  }
  // shell2 pairs with z holes: every monitor of the plan clear of the holes' planes (their single steps copy nothing out) — a DFT
  // monitor inside one SEGMENT (an interval, extended to the grid's end below the first / above the last), a time monitor inside one interval
  bool plan_clear_of_holes(const F2Plan& pl, const ZPlan& zp) {
    auto inside = [&](const Monitor& m, bool segment) {
      for (int i = 0; i < zp.n; ++i) {
        const int lo = (segment && i == 0) ? 0 : zp.a[i], hi = (segment && i == zp.n - 1) ? nz : zp.b[i];
        if (m.box.lo2 >= lo && m.box.lo2 + m.box.nz <= hi) return true;
      }
      return false;
    };
    for (int q : pl.mons) if (!inside(h->mons[(size_t)q], false)) return false;
    for (int q : pl.dfts) if (!inside(h->mons[(size_t)q], true)) return false;
    // (a periodic y: the single steps of the rows next to the wrap copy nothing out either)
    if (h->cfg.bc[2] == FDTD_BC_PERIODIC)
      for (int q : pl.dfts) {
        const Monitor& m = h->mons[(size_t)q];
        if (m.box.lo1 < 2 || m.box.lo1 + m.box.ny > h->g.ny - 2) return false;
      }
    return true;
  }
  // every monitor of the pair's plan inside ONE interval of the bulk's planes (the sweep copies the middle step out only there)
  bool plan_in_bulk(const F2Plan& pl, const ZPlan& zp) {
    auto inside = [&](const Monitor& m) {
      for (int i = 0; i < zp.n; ++i) if (m.box.lo2 >= zp.a[i] && m.box.lo2 + m.box.nz <= zp.b[i]) return true;
      return false;
    };
    for (int q : pl.mons) if (!inside(h->mons[(size_t)q])) return false;
    for (int q : pl.dfts) if (!inside(h->mons[(size_t)q])) return false;
    return true;
  }
  // steps n and n + 1 as ONE sweep, and in which form?  (fdtd_kernels2.hpp; no decay check on the middle step, sources all alive or all
  // spent, every monitor that records at n or n + 1 a small time monitor the sweep can sample.)  The order of the attempts: the shell2
  // form; shell2 with the source lists' planes as z holes; back to the single-step shell where the plan is not clear of the holes; the
  // shell's own source-hole plan; plain.  Fills f2_plan for the form it returns.
  PairChoice choose_pair() {
    const PairChoice none;
    if (!(fused && (f2_ok || f2s_ok || s2_ok) && two_steps_free(n))) return none;
    PairChoice c;
    int why = fused2_sources_why_not(h, n, &c.src_alive);
    // lists the node table cannot hold, while they inject: paged source terms in the sweep, the seam kernel and the shell's boxes —
    // plain pairs and shell2 pairs without z holes (a periodic y's wrap rows take single steps: the round-5 forms there)
    bool spg = false;
    if (why != 0 && spg_ok && (why == FDTD_F2_OFF_TFSF || why == FDTD_F2_OFF_SOURCES || why == FDTD_F2_OFF_SEAM_SOURCE)) {
      const bool s2_form = s2_ok && zp_s2.ok && zp_s2.n == 1 && h->cfg.bc[2] != FDTD_BC_PERIODIC;
      if (s2_form || f2_ok) { spg = true; why = 0; c.src_alive = false; }
    }
    // shell2 form: the boxes apply no sources — lists that inject must lie deep inside the bulk
    if (s2_ok && why == 0 && (!c.src_alive || s2_deep || spg)) { c.form = PairForm::Shell2; c.zp = &zp_s2; }
    else if (s2_ok && zp_s2h.ok && (why != 0 || c.src_alive)) {
      // lists that inject and that the sweeps cannot apply themselves (too many nodes, nodes inside the shell, TFSF corrections): their
      // planes take single steps as z holes; nothing is injected by the sweeps (the table of a pair whose lists are spent)
      c.form = PairForm::Shell2Holes; c.zp = &zp_s2h; why = 0; c.src_alive = false;
    } else if (!f2_ok && !f2s_ok) { if (why) h->f2_dyn_reason = why; return none; }
    if (c.form != PairForm::None && !(fused2_plan(h, n, &f2_plan, sg.o0, sg.o1, true) && plan_clear_of_holes(f2_plan, *c.zp))) {
      if (!f2s_ok) return none;
      c.form = PairForm::None;                             // (the single-step shell may still take it — judged below)
      why = fused2_sources_why_not(h, n, &c.src_alive);
    }
    if (c.form == PairForm::None) {
      c.form = f2s_ok ? PairForm::Shell : PairForm::Plain;
      c.zp = &zp_base;
      // lists that inject and that the sweep cannot apply itself: a shell pair whose bulk leaves their planes to the shell
      if (why && f2s_ok && zp_src.ok) { why = 0; c.src_alive = false; c.zp = &zp_src; }
      if (why) h->f2_dyn_reason = why;
      if (!(why == 0 && fused2_plan(h, n, &f2_plan, f2s_ok ? sg.o0 : nullptr, f2s_ok ? sg.o1 : nullptr) &&
            (!f2s_ok || plan_in_bulk(f2_plan, *c.zp)))) return none;
    }
    const bool plain_or_s2 = c.form == PairForm::Plain || c.form == PairForm::Shell2;
    c.disp = !h->ade.empty() && h->disp.state == 1 && plain_or_s2 && (c.form == PairForm::Plain || s2_disp);
    c.spg = spg && plain_or_s2;
    return c;
  }
  // the step about to be issued: does a monitor record at it (rec), can steps n and n + 1 go out as one sweep, in which form (pc)
  int begin_step() {
    n = h->step;
    rec = !fused_multi && rec_at(h, n);
    if (rec) flush_seams(h, st);
    if (rec && multi) {
      HIPCHK(h, hipStreamWaitEvent(st, h->ev_e_bnd, 0));
      HIPCHK(h, hipStreamWaitEvent(st, h->ev_h_bnd, 0));
    }
    pc = choose_pair();
    // (with H-side sources the monitors of a pair still take E^n and H^{n-1/2} here: those sources change H^{n-1/2} before the
    //  sweep, and pair_record reads the set afterwards)
    if (rec) record_monitors(h, n, false, st, (pc.form != PairForm::None && !h_terms_in_front(h)) ? &f2_plan : nullptr);
    if (rec && multi) {
      // The record reads H^{n-1/2} of the top plane, which the comm stream is about to advance (its H-side corrections and
      // update of that plane wait for the E interior of the LAST step only): it must let the record finish first.  Found by
      // scripts/fuzz_variants.py on the device (round 4): a volume time monitor reaching the slab's top plane came back with
      // that plane's H half-sample taken during / after the update, in one run out of a few.
      if (!h->ev_rec) HIPCHK(h, hipEventCreateWithFlags(&h->ev_rec, hipEventDisableTiming));
      HIPCHK(h, hipEventRecord(h->ev_rec, st));
      HIPCHK(h, hipStreamWaitEvent(cs, h->ev_rec, 0));
    }
    return 0;
  }
  // steps n and n + 1 of a z-slab rank (entry and exit state: "primed"; slab_rank_step decides and describes the form).  On a rank that
  // carries CPML (p.shell2):
  //   st: the bulk (sgm: the CPML-free box, two or more planes from a cut) as ONE clipped two-step sweep, set A -> set B
  //   cs: the two planes next to each cut as a z hole — step one A -> T over the hole grown by one plane (psi: current sets ->
  //       temporary sets), its E-side / the next H-side source terms, the planes (and the H-side psi of the top plane, temporary
  //       set) travel; step two T -> B (psi: temporary -> the other sets), source terms, the planes travel again — the messages of
  //       two single steps, in their order.
  //   st, behind the bulk: the shell's boxes (x strips, y / z slabs over the planes clear of the cuts) by shell2_step_kernel, A -> B,
  //       psi current -> other sets.
  // No launch reads what another one of the pair writes; the next step's edges (ev_e_bnd, ev_e_int) order it behind both streams.
  // On a rank without CPML: the bulk is every plane two or more from a cut, there are no boxes and no psi; the rest is the same.
  // (host order: the long bulk sweep is handed to the device before the comm stream's launches — its dozen launches and two RCCL groups
  //  take the host longer to issue than the device needs for them; issued first they left the device idle for 30 us per pair in front
  //  of the bulk, profiles/r4e)
  int slab_pair(const F2Table* tb, const SlabPair& p) {
    const int bl = nb_lo ? 2 : 0, bh = nb_hi ? 2 : 0;
    const FieldP B = h->f2, T = h->f3;
    HIPCHK(h, hipStreamWaitEvent(cs, h->ev_e_int, 0));
    HIPCHK(h, hipStreamWaitEvent(st, h->ev_e_bnd, 0));
    bool s2done = false;
    Shell2Box boxes[kShell2MaxBoxes];
    const int nb = p.shell2 ? shell2_boxes(h, sgm, boxes, bl, nz - bh) : 0;
    const PmlP* pm2 = p.shell2 ? h->pml_blk2[h->pml_parity][h->pml_e_parity] : nullptr;       // the boxes' parameter block
    const bool boxes_first = p.shell2 && h->slab_boxes_first, boxes_behind = p.shell2 && !h->slab_boxes_first;
    // Round 6: the boxes go out IN FRONT of the bulk on st (FDTD_OPT_SLAB_BOXES_FIRST, default).  Behind it (round 5) they ran alone
    // on the machine for 87 us of a 362 us pair of a 64-plane slab while the hole's first step, beside the bulk's single round of
    // one-per-CU workgroups, crawled for 160 us on the CUs the bulk left (kernel timeline profiles/r6/r6tr_timeline_p2.txt); in front,
    // boxes and hole share the machine, then the bulk runs beside the exchanges and the hole's second step.
    // (2: on a third stream beside both — the boxes read set A and their own psi sets, write their own cells of set B: they wait for what
    //  st and cs waited for, and st waits for them before it marks the pair's interior done)
    // Measured (profiles/r6/r6b3_slab_boxes_third_stream.jsonl, 512 x 512 x nz with CPML on x / y, three rounds interleaved): 128 planes 0.3226 ->
    // 0.3175 ms per step, 256 planes 0.571 -> 0.561 — but 64 planes 0.164 -> 0.213: beside a bulk of ONE round of one-per-CU workgroups the
    // boxes and the hole's first step crawl on the CUs the bulk left, and st waits for the boxes.  Hence 3: by the slab's planes.
    bool third = (h->slab_boxes_first == 2 || (h->slab_boxes_first == 3 && nz >= 96)) && nb > 0 && !h->streams_shared && !h->debug_sync;
    if (third && !h->box_stream_tried && make_box_stream(h)) return -1;
    third = third && h->box_stream != nullptr;
    if (third) {
      HIPCHK(h, hipEventRecord(h->ev_box_in, st));                            // (everything st has issued: the last pair's interior)
      HIPCHK(h, hipStreamWaitEvent(h->box_stream, h->ev_box_in, 0));
      HIPCHK(h, hipStreamWaitEvent(h->box_stream, h->ev_e_bnd, 0));
      launch_shell2_boxes(h, boxes, nb, pm2, h->box_stream, tb);
      HIPCHK(h, hipEventRecord(h->ev_box, h->box_stream));
    } else if (boxes_first) launch_shell2_boxes(h, boxes, nb, pm2, st, tb);
    // bulk: both steps in one sweep, set A -> set B
    if (launch_fused2(h, n, st, tb, &s2done, nullptr, &p.clip)) return -1;
    // hole, step one: the planes next to the cuts and one more (what step two differentiates), set A -> set T
    if (launch_fused_range(h, cs, {.k0 = 0, .k1 = bl ? bl + 1 : 0, .pml = p.pml, .k2_0 = bh ? nz - bh - 1 : nz, .k2_1 = nz, .edge = p.edge, .sh = &p.s1})) return -1;
    HIPCHK(h, hipEventRecord(h->ev_h_bnd, cs));
    if (bl) { launch_sources(h, true, n, 0, bl + 1, cs, false, &T); launch_sources(h, false, n + 1, 0, bl + 1, cs, false, &T); }
    if (bh) { launch_sources(h, true, n, nz - bh - 1, nz, cs, false, &T); launch_sources(h, false, n + 1, nz - bh - 1, nz, cs, false, &T); }
    if (exchange_fused_all(h, cs, p.psi, &T, p.psi_set[0])) return -1;                 // what the neighbours expect after step n
    // hole, step two: set T -> set B; corrections of step n + 1 (E side) and n + 2 (H side), then its planes travel
    if (launch_fused_range(h, cs, {.k0 = 0, .k1 = bl, .pml = p.pml, .k2_0 = nz - bh, .k2_1 = nz, .edge = p.edge, .sh = &p.s2})) return -1;
    if (bl) { launch_sources(h, true, n + 1, 0, bl, cs, false, &B); launch_sources(h, false, n + 2, 0, bl, cs, false, &B); }
    if (bh) { launch_sources(h, true, n + 1, nz - bh, nz, cs, false, &B); launch_sources(h, false, n + 2, nz - bh, nz, cs, false, &B); }
    HIPCHK(h, hipEventRecord(h->ev_e_bnd, cs));
    if (exchange_fused_all(h, cs, p.psi, &B, p.psi_set[1])) return -1;
    // (not on cs: it carries what the neighbours wait for — behind the hole's steps and the two exchanges the boxes made cs the longer
    //  stream of a thin slab: 64 planes 0.232 -> 0.205 ms per step, 128 planes 0.500 -> 0.460, profiles/r5/r5zb)
    if (boxes_behind) launch_shell2_boxes(h, boxes, nb, pm2, st, tb);
    if (third) HIPCHK(h, hipStreamWaitEvent(st, h->ev_box, 0));
    swap_sets(h);                                                            // h->f = B: E^{n+2}, H^{n+3/2}
    if (p.shell2) { swap_psi_h(h, 7); swap_psi_e(h); h->shell2_pairs++; }
    launch_sources(h, true, n + 1, bl, nz - bh, st);
    launch_sources(h, false, n + 2, bl, nz - bh, st);
    HIPCHK(h, hipEventRecord(h->ev_e_int, st));
    h->fused2_pairs++;
    h->step = n + 2;
    return 1;
  }
  // one step — or, where it can, a step pair — of a z-slab rank on the pipelined fused schedule (header comment: setup; slab pair: below).
  // -> 1: a pair was taken (two steps, no decay check due), 0: one step, < 0: error
  int slab_rank_step() {
    if (!primed && prime(n)) return -1;
    // ---- slab pair: steps n and n + 1 of a z-slab rank -----------------------------------------------------------------
    // The two-step sweep advances the planes two or more away from a neighbour face (it reads the slab's own planes
    // only: no ghost plane, no dependence on the wire); the two planes next to a neighbour face — its shell — take two
    // single steps on the comm stream, through the third set, and ship their planes after EACH of them: the messages a
    // neighbour receives are those of two single steps, in the same order (a rank may take a pair while its neighbour
    // takes single steps).  Same kernels and formulas: the same bits (tests/test_dist_gloo.py).  Entry and exit state:
    // "primed" (above).  Pairs keep clear of monitor records, decay checks and the end of the run (joined tails).
    // (CPML-carrying ranks, f2mc: lists that inject must lie deep inside the bulk — the boxes apply no sources)
    bool alive = false;
    if ((f2m_ok || f2mc_ok) && steps_free(n, 3, {n, n + 1, n + 2}) && fused2_sources_why_not(h, n, &alive) == 0 &&
        (f2m_ok || !alive || f2mc_deep)) {
      F2Plan none;
      const F2Table* tb = fused2_table(h, none, alive);
      if (!tb) return -1;
      const FieldP A = h->f, B = h->f2, T = h->f3;
      if (f2m_ok) return slab_pair(tb, {.clip = {0, h->g.nx, 0, h->g.ny, nb_lo ? 2 : 0, nz - (nb_hi ? 2 : 0)}, .pml = 0, .edge = false,
                                        .s1 = {A, T, 0, 0, 0}, .s2 = {T, B, 0, 0, 0}, .psi = false, .psi_set = {0, 0}, .shell2 = false});
      const int hp = h->pml_parity, ep = h->pml_e_parity;
      return slab_pair(tb, {.clip = {sgm.o0[0], sgm.o1[0], sgm.o0[1], sgm.o1[1], sgm.o0[2], sgm.o1[2]}, .pml = pml_in_m, .edge = true,
                            .s1 = {A, T, hp, 0, 0, h->pml_blk_hole[0][hp][ep]}, .s2 = {T, B, hp, 0, 0, h->pml_blk_hole[1][hp][ep]},
                            .psi = psi_ghosts, .psi_set = {1, 2}, .shell2 = true});
    }
    const bool decay_step = decay_at(n + 1);
    const bool last = (done + 1 == n_steps) || decay_step;
    // sweeps: boundary chunks (one launch) on cs, interior on st
    HIPCHK(h, hipStreamWaitEvent(cs, h->ev_e_int, 0));
    // (the boundary chunks lie clear of the z slabs: their launch carries x / y at most)
    const int pml_b = pml_in_m & 3;
    if (b_lo > 0 && b_hi > 0) { if (launch_fused_range(h, cs, {.k0 = 0, .k1 = b_lo, .pml = pml_b, .k2_0 = nz - b_hi, .k2_1 = nz})) return -1; }
    else if (b_lo > 0) { if (launch_fused_range(h, cs, {.k0 = 0, .k1 = b_lo, .pml = pml_b})) return -1; }
    else if (b_hi > 0) { if (launch_fused_range(h, cs, {.k0 = nz - b_hi, .k1 = nz, .pml = pml_b})) return -1; }
    HIPCHK(h, hipEventRecord(h->ev_h_bnd, cs));
    HIPCHK(h, hipStreamWaitEvent(st, h->ev_e_bnd, 0));
    if ((pml_in_m & 6) == 0) {
      if (launch_fused_range(h, st, {.k0 = b_lo, .k1 = nz - b_hi, .pml = pml_in_m})) return -1;
    } else {
      // interior planes by tile class, as on one GPU (all three on the main stream: the other one ships ghost planes)
      const int ki = b_lo, ke = nz - b_hi;
      const TileSplit t = tile_split(pml_in_m, ki, ke);
      // (all on the main stream.  Edge launches on a third stream were tried: no gain, and an engine with three
      //  streams pushed the next engine of the process onto shared hardware queues — its two streams serialised,
      //  3x slower steps, profiles/r04r)
      if ((t.za > ki || t.zc < ke) && launch_fused_range(h, st, {.k0 = ki, .k1 = t.za, .pml = pml_in_m, .k2_0 = t.zc, .k2_1 = ke, .edge = true})) return -1;
      if (launch_fused_range(h, st, t.edge_rows(pml_in_m))) return -1;
      if (launch_fused_range(h, st, t.middle_rows(pml_in_m))) return -1;
    }
    swap_sets(h);
    swap_psi_h(h, pml_in_m);
    const bool rec_post = rec_at(h, n);
    if (rec_post || last || rec_at(h, n + 1)) {
      // joined tail: everything after the sweeps on st
      HIPCHK(h, hipStreamWaitEvent(st, h->ev_h_bnd, 0));
      if (rec_post) record_monitors(h, n, true, st);
      e_post(n, 0, nz, st, false);
      advance_tfsf_aux(h, true, n, st, false);
      advance_tfsf_aux(h, true, n, st, true);
      primed = false;
      if (!last && prime(n + 1)) return -1;
      if (last) {           // leave both streams joined; the next step (or run) primes again
        HIPCHK(h, hipEventRecord(h->ev_e_int, st));
        HIPCHK(h, hipStreamWaitEvent(cs, h->ev_e_int, 0));
        HIPCHK(h, hipEventRecord(h->ev_e_bnd, cs));
      }
    } else {
      e_post(n, 0, b_lo, cs, true);
      e_post(n, nz - b_hi, nz, cs, true);
      advance_tfsf_aux(h, true, n, cs, true);
      h_pre(n + 1, 0, b_lo, cs, true);
      h_pre(n + 1, nz - b_hi, nz, cs, true);
      advance_tfsf_aux(h, false, n + 1, cs, true);
      HIPCHK(h, hipEventRecord(h->ev_e_bnd, cs));
      if (exchange_fused_all(h, cs, psi_ghosts)) return -1;
      e_post(n, b_lo, nz - b_hi, st, false);
      advance_tfsf_aux(h, true, n, st, false);
      h_pre(n + 1, b_lo, nz - b_hi, st, false);
      advance_tfsf_aux(h, false, n + 1, st, false);
      HIPCHK(h, hipEventRecord(h->ev_e_int, st));
    }
    h->step = n + 1;
    return 0;
  }
  // steps n and n + 1 of a run without CPML as ONE two-step sweep, all on st: set A -> set B, swap
  int plain_pair(const F2Table* tb) {
    bool sources2_done = false, damp2_done = true;
    launch_sources(h, false, n, 0, nz, st);              // H-side sources of step n act on H^{n-1/2}, as before a single step
    if (pc.spg) spg_fill(h, n, st);                      // (the other source terms of the pair into paged storage, the incident grids through both steps)
    // deferred seam repair: only when the NEXT two steps are known to be a plain pair of this run with nothing in front of, between or behind
    // the two sweeps that reads or writes the fields — no record, no decay check, no H-side source launch, no ghost planes to copy
    // (four steps free from n on: this pair was chosen with no decay check at n + 1 — choose_pair — so that term adds nothing)
    const bool defer_ok = steps_free(n, 4, {n + 1, n + 2, n + 3}) && !pc.disp && !pc.spg && h->tfsf.empty() && h->src_h_nodes == 0 && h->cfg.bc[4] != FDTD_BC_PERIODIC && !multi &&
                          !h->step_dev_mode && !h->debug_sync;
    if (launch_fused2(h, n, st, tb, &sources2_done, &damp2_done, nullptr, pc.disp, false, pc.spg ? spg_params(h) : SrcP{}, defer_ok)) return -1;
    pair_record(h, tb, n, st);                           // (H^{n+3/2} is not touched by the E-side sources that follow)
    if (rec_at(h, n + 1)) record_monitors(h, n + 1, true, st);      // DFT records at the middle step: their H terms, from the write set
    if (!sources2_done) launch_sources(h, true, n + 1, 0, nz, st);
    if (h->has_damp && !damp2_done) launch_damp(h, true, 0, nz, st);
    if (pc.disp) launch_ade2(h, st);                     // (the ADE update of step n + 1 follows its sources and damping, as launch_ade does)
    fill_ghost_fused(h, st);
    return 0;
  }
  // one step of the two-pass kernels (H pass, E pass; odd row lengths, FDTD_VARIANT_ZMARCH, z-slab ranks on the AUTO variant): interior on st,
  // the plane next to a neighbour face and the exchanges on cs; edges: ev_e_int, ev_e_bnd, ev_h_int, ev_h_bnd (setup_schedules)
  int two_pass_step() {
    // ---------------- H phase ----------------
    const int h_top = (multi && nb_hi) ? nz - 1 : nz;      // planes [0, h_top) on st, [h_top, nz) on cs
    const bool mirrors = h->mirror_wall[0] >= 0 || h->mirror_wall[1] >= 0 || h->mirror_wall[2] >= 0;
    if (multi && mirrors) {
      // PMC plus walls on a z-slab rank: the images of ALL planes are refreshed on the main stream before either stream goes on —
      // its H pass differentiates E of the top plane (image columns included: the update of an image cell feeds the wall's own
      // unknowns in the same step), so the comm stream must not refresh that plane beside it (a race the device showed in one
      // visit out of three, tests/test_gpu_parity.py)
      HIPCHK(h, hipStreamWaitEvent(st, h->ev_e_bnd, 0));
      fill_mirror(h, st, 0, nz);
      if (!h->ev_rec) HIPCHK(h, hipEventCreateWithFlags(&h->ev_rec, hipEventDisableTiming));
      HIPCHK(h, hipEventRecord(h->ev_rec, st));
      HIPCHK(h, hipStreamWaitEvent(cs, h->ev_rec, 0));
    }
    if (multi && nb_hi) {
      HIPCHK(h, hipStreamWaitEvent(cs, h->ev_e_int, 0));
      h_side_terms(h, n, h_top, nz, cs);
      launch_h_main(h, h_top, nz, cs);
      HIPCHK(h, hipEventRecord(h->ev_h_bnd, cs));
    }
    if (multi) HIPCHK(h, hipStreamWaitEvent(st, h->ev_e_bnd, 0));
    if (!multi) fill_mirror(h, st, 0, nz);
    h_side_terms(h, n, 0, h_top, st);
    launch_h_main(h, 0, h_top, st);
    advance_tfsf_aux(h, false, n, st);
    if (multi) {
      HIPCHK(h, hipEventRecord(h->ev_h_int, st));
      if (!nb_hi) HIPCHK(h, hipStreamWaitEvent(cs, h->ev_h_int, 0));
      HIPCHK(h, hipStreamWaitEvent(cs, h->ev_e_int, 0));     // WAR: ghost(-1) was read by the last E pass
      if (exchange(h, false, cs)) return -1;
    }
    if (!multi || !nb_lo) fill_ghost_h(h, st);   // physical z-min face of this slab (PMC / periodic)
    if (rec) {
      if (multi) HIPCHK(h, hipStreamWaitEvent(st, h->ev_h_bnd, 0));
      record_monitors(h, n, true, st);
    }
    // ---------------- E phase ----------------
    const int e_bot = (multi && nb_lo) ? 1 : 0;            // planes [0, e_bot) on cs, [e_bot, nz) on st
    if (multi && nb_lo) {
      HIPCHK(h, hipStreamWaitEvent(cs, h->ev_h_int, 0));
      launch_e_main(h, 0, e_bot, cs);
      e_side_terms(h, n, 0, e_bot, cs, false);
      HIPCHK(h, hipEventRecord(h->ev_e_bnd, cs));
    }
    if (multi && nb_hi) HIPCHK(h, hipStreamWaitEvent(st, h->ev_h_bnd, 0));
    aniso_save(h, st);                     // (these kernels update E in place: E^n of the nodes around fully anisotropic cells first)
    modulation_save(h, st);
    nonlinear_save(h, st);
    launch_e_main(h, e_bot, nz, st);
    e_side_terms(h, n, e_bot, nz, st, !multi);     // (one GPU: [e_bot, nz) is the whole grid; a z-slab rank carries no whole-grid lists — setup)
    advance_tfsf_aux(h, true, n, st);
    if (multi) {
      HIPCHK(h, hipEventRecord(h->ev_e_int, st));
      if (!nb_lo) HIPCHK(h, hipStreamWaitEvent(cs, h->ev_e_int, 0));
      HIPCHK(h, hipStreamWaitEvent(cs, h->ev_h_int, 0));     // WAR: ghost(nz) was read by this H pass
      if (exchange(h, true, cs)) return -1;
    }
    if (!multi || !nb_hi) fill_ghost_e(h, st);   // physical z-max face of this slab (periodic)
    h->step = n + 1;
    return 0;
  }
  // field decay / divergence every decay_every steps (joins the streams; the only host synchronisation of the loop).  -> 1: the run ends here
  int decay_check() {
    if (!decay_at(h->step)) return 0;
    if (multi) HIPCHK(h, hipStreamWaitEvent(st, h->ev_e_bnd, 0));
    double en = 0.0;
    if (eval_energy(h, st, &en)) return -1;
    if (multi && allreduce_energy(h, &en, cs)) return -1;
    return decay_verdict({h}, en, progress, user);
  }
  // joins the streams, reads the timers
  int finish() {
    flush_seams(h, st);          // (a run never returns with stale seam columns)
    ring_drain(h, st);           // (nor with records waiting in their rings)
    if (multi) {
      HIPCHK(h, hipStreamWaitEvent(st, h->ev_e_bnd, 0));
      HIPCHK(h, hipStreamWaitEvent(st, h->ev_h_bnd, 0));
    }
    HIPCHK(h, hipEventRecord(h->ev1, st));
    HIPCHK(h, hipStreamSynchronize(st));
    HIPCHK(h, hipStreamSynchronize(cs));
    for (hipEvent_t e : tb_ev) hipEventDestroy(e);
    for (const GraphRec& r : graphs) hipGraphExecDestroy(r.exec);
    HIPCHK(h, hipGetLastError());
    if (run_stats({h})) return -1;
    for (size_t i = 0; i < h->kev_kind.size(); ++i) {
      float t = 0.f;
      if (hipEventElapsedTime(&t, h->kev[2 * i], h->kev[2 * i + 1]) != hipSuccess) continue;
      if (h->kev_kind[i] == 0) { h->stats.h_kernel_ms += t; h->stats.h_kernel_launches++; }
      else if (h->kev_kind[i] == 1) { h->stats.e_kernel_ms += t; h->stats.e_kernel_launches++; }
      else if (h->kev_kind[i] == 3) { h->stats.shell_kernel_ms += t; h->stats.shell_kernel_launches++; }
      else if (h->kev_kind[i] == 4) { h->stats.seam_kernel_ms += t; h->stats.seam_kernel_launches++; }
      else if (h->kev_kind[i] == 5) h->seam_flush_ms += t;
      else { h->stats.fused_kernel_ms += t; h->stats.fused_kernel_launches++; }
    }
    return 0;
  }
  int loop() {
    for (; done < n_steps; ++done) {
      if (begin_step()) return -1;
      if (h->seam_pending && pc.form != PairForm::Plain) flush_seams(h, st);      // (not the plain pair that was expected)
      if (fused_multi) {
        const int rc = slab_rank_step();
        if (rc < 0) return -1;
        if (rc > 0) { ++done; continue; }
      } else if (!fused) {
        if (two_pass_step()) return -1;
      } else {
        int took = 0;                                        // steps issued
        if (tb_ok && !rec && two_steps_free(n, {n + 1})) { if (tb_pair(n)) return -1; took = 2; }
        else if (pc.form != PairForm::None) {
          const F2Table* tb = fused2_table(h, f2_plan, pc.src_alive);
          if (!tb) return -1;
          const bool s2 = pc.form == PairForm::Shell2 || pc.form == PairForm::Shell2Holes;
          int rc;
          switch (pc.form) {
            case PairForm::Plain: rc = plain_pair(tb); break;
            case PairForm::Shell: rc = shell_pair(n, tb, *pc.zp); break;
            default: rc = shell2_pair(n, tb, *pc.zp); break;      // Shell2, Shell2Holes
          }
          if (rc) return -1;
          h->fused2_pairs++;
          if (pc.form != PairForm::Plain) h->shell_pairs++;
          if (s2) h->shell2_pairs++;
          took = 2;
        } else if (graph_ok && !rec && two_steps_free(n, {n + 1}) && sources_alive(n + 1)) {
          const int grc = graph_pair(n);                     // (1: capture not available — this step directly, no more attempts)
          if (grc < 0) return -1;
          if (grc == 0) took = 2;
        }
        if (!took) { if (fused_one(n, rec)) return -1; took = 1; }
        h->step = n + took;
        if (took == 2) ++done;                               // (the loop header counts the first step)
      }
      sync_point();
      const int dc = decay_check();
      if (dc < 0) return -1;
      if (dc > 0) { ++done; break; }
    }
    return 0;
  }
};
