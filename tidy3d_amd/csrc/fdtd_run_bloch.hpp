// The run loop of fdtd_run_bloch: a fragment of fdtd_capi.hip, included there once, inside its unnamed namespace, behind fdtd_run.hpp
// (whose free functions — run_begin, rec_at, default_shape_wgs, allreduce_energy, decay_verdict, run_stats — it shares with Run).
// Not a stand-alone header.
// Complex (Bloch-periodic) fields: two solvers carry Re and Im of the same simulation (identical grid,
// media, CPML, ADE and monitors; the Im solver's source weights are the Re solver's times -i) and are
// stepped together on the Re solver's stream; they only meet in the ghost fills (fdtd_kernels.hpp) and in the fully anisotropic
// coupling.  phase[a] = 2 pi bloch_vec of axis a (ref boundary.py:55-79 bloch_phase).  n_real[a] > 0 (a = x, y): the
// axis carries ghost cells at device index 0 and n_real[a] + 1 (the host builds the grid that way and
// declares PEC walls); z uses its ghost planes when the z faces are FDTD_BC_PERIODIC.  One GPU; the
// fused sweep unless the handles ask for the two-pass kernels.
// One `BlochRun` object per call, in the shape of Run: setup, step (one single step of both parts; the order of its correction
// launches is h_side_terms / e_side_terms, fdtd_capi.hip), decay_check, finish.  Everything is issued on ONE stream, st.

struct BlochRun {
  FdtdSolver *hr, *hi;
  int64_t n_steps;
  const double* phase;
  const int* n_real;
  FdtdProgressFn progress;
  void* user;
  // the run's configuration (setup)
  FdtdSolver* both[2] = {nullptr, nullptr};
  bool aniso = false, multi = false, nb_lo = false, nb_hi = false, per_z = false, fused = false;
  int nz = 0;
  long long pc = 0;
  hipStream_t st = nullptr;
  float cph[3] = {}, sph[3] = {};
  AnisoPhaseTab wrap_tab{};            // (cos, sin) of each wrap code of the coupling lists
  int lo_rank = 0, hi_rank = 0;
  bool wrap_lo = false, wrap_hi = false;

  // checks, the variant (fused / two-pass, one GPU / z-slab rank), the tile-shape probe, the phases
  int setup() {
    for (const FdtdSolver* hh : {hr, hi}) if (refuse_whole_grid_monitors(hr, hh, "fdtd_run_bloch", true)) return -1;
    if (hi->comm) return fail(hr, "fdtd_run_bloch: the communicator of a z-slab belongs to the first (real-part) handle");
    // whole-grid lists (kListKind): the same on both handles or refused; the Re handle's anisotropic lists (wrap codes included) drive both parts
    if (check_bloch_lists(hr, hi)) return -1;
    aniso = n_lists(hr, kAniso) > 0;
    for (int a = 0; a < 3; ++a)
      if (hr->mirror_wall[a] >= 0 || hi->mirror_wall[a] >= 0) return fail(hr, "fdtd_run_bloch: PMC on a plus face is not available together with Bloch boundaries");
    // z-slab decomposition (hr->comm): both parts exchange their ghost planes through the real-part handle's
    // communicator; the planes that wrap around a Bloch z axis (rank n-1 <-> rank 0) are rotated by exp(-+ i phi_z)
    // on arrival.  Two-pass kernels, exchanges on the step stream (correct by construction; not overlapped).
    multi = hr->comm != nullptr;
    nb_lo = hr->cfg.bc[4] == FDTD_BC_NEIGHBOR, nb_hi = hr->cfg.bc[5] == FDTD_BC_NEIGHBOR;
    if ((nb_lo || nb_hi) && !multi) return fail(hr, "fdtd_run_bloch: neighbour faces need fdtd_comm_init on the first handle");
    if (multi && refuse_lists_on_z_slabs(hr, hr, "fdtd_run_bloch")) return -1;
    if (hi->cfg.bc[4] != hr->cfg.bc[4] || hi->cfg.bc[5] != hr->cfg.bc[5])
      return fail(hr, "fdtd_run_bloch: the two solvers must have the same z faces");
    if (hr->g.nx != hi->g.nx || hr->g.ny != hi->g.ny || hr->g.nz != hi->g.nz || hr->cfg.device != hi->cfg.device ||
        hr->mons.size() != hi->mons.size() || hr->step != hi->step)
      return fail(hr, "fdtd_run_bloch: the two solvers must describe the same simulation");
    const GridP& g = hr->g;
    nz = g.nz;
    const int N[3] = {g.nx, g.ny, nz};
    for (int a = 0; a < 2; ++a)
      if (n_real[a] < 0 || (n_real[a] > 0 && n_real[a] + 2 > N[a]))
        return fail(hr, "fdtd_run_bloch: axis %d has %d cells, cannot hold %d real cells + 2 ghost cells", a, N[a], n_real[a]);
    HIPCHK(hr, hipSetDevice(hr->cfg.device));
    st = hr->stream;
    HIPCHK(hr, hipStreamSynchronize(hi->stream));
    both[0] = hr, both[1] = hi;
    hr->bloch_pair = hi->bloch_pair = true;
    if (run_begin({hr, hi}, st)) return -1;
    per_z = hr->cfg.bc[4] == FDTD_BC_PERIODIC;
    // (a wide material table keeps the two-pass kernels here, whatever the variant asked for: Run::setup lets FDTD_VARIANT_FUSED read it)
    fused = !multi && !hr->mat4b && (g.nx % 4 == 0) && hr->rows_f <= 15 &&
            (hr->cfg.variant == FDTD_VARIANT_FUSED || hr->cfg.variant == FDTD_VARIANT_AUTO);
    if (fused) for (FdtdSolver* h : both) if (ensure_second_set(h)) return -1;
    // Tile-shape probe: the rule of fdtd_run with this run's own threshold and placement of the size check (kProbeBelowWgsBloch,
    // fdtd_run.hpp, says how the two differ); the shape chosen for the Re handle goes to both
    if (fused && !hr->tuned && !hr->user_geometry && !hi->user_geometry && (n_cells(hr) >= (1LL << 20) || hr->autotune == 2) &&
        (default_shape_wgs(hr) < kProbeBelowWgsBloch || hr->autotune)) {
      if (autotune_fused(hr, st)) return -1;
      hi->rows_f = hr->rows_f; hi->zchunk_f = hr->zchunk_f; hi->tuned = true;
    }
    for (int a = 0; a < 3; ++a) { cph[a] = (float)std::cos(phase[a]); sph[a] = (float)std::sin(phase[a]); }
    // (cos, sin) of each wrap code of the coupling lists: the sum of the phases the ghost fills apply on the axes it crosses
    if (aniso) {
      const double ph[3] = {n_real[0] > 0 ? phase[0] : 0.0, n_real[1] > 0 ? phase[1] : 0.0, per_z ? phase[2] : 0.0};
      for (int c = 0; c < kWrapCodes; ++c) {
        double p = 0.0;
        for (int a = 0; a < 3; ++a) {
          const int w = (c >> (2 * a)) & 3;
          p += w == 1 ? ph[a] : (w == 2 ? -ph[a] : 0.0);
        }
        wrap_tab.r[c] = make_float2((float)std::cos(p), (float)std::sin(p));
      }
    }
    pc = plane_cells(hr);
    lo_rank = (hr->rank - 1 + hr->n_ranks) % hr->n_ranks, hi_rank = (hr->rank + 1) % hr->n_ranks;
    wrap_lo = nb_lo && hr->rank == 0, wrap_hi = nb_hi && hr->rank == hr->n_ranks - 1;
    return 0;
  }
  // (pointers are taken at call time: the fused sweep swaps the field sets every step)
  Cplx6P six() { Cplx6P F; for (int c = 0; c < 6; ++c) { F.f[c].re = field_ptr(hr, c); F.f[c].im = field_ptr(hi, c); } return F; }
  void fill_xy() {                // y first, then x over all rows (ghost rows included): corners get both phases
    const GridP& g = hr->g;
    for (int a = 1; a >= 0; --a) {
      if (n_real[a] <= 0) continue;
      const long long cells = (long long)(a == 0 ? g.ny : g.nx) * nz;
      hipLaunchKernelGGL(bloch_ghost_fill_kernel, dim3(nblk(cells)), dim3(256), 0, st, g, a, n_real[a], six(), cph[a], sph[a], nz);
    }
  }
  void plane(int c, long long dst_plane, long long src_plane, float s) {
    hipLaunchKernelGGL(bloch_plane_kernel, dim3(nblk(pc)), dim3(256), 0, st, field_ptr(hr, c) + dst_plane * pc,
                       field_ptr(hi, c) + dst_plane * pc, (const float*)(field_ptr(hr, c) + src_plane * pc),
                       (const float*)(field_ptr(hi, c) + src_plane * pc), cph[2], s, pc);
  }
  // ghost-plane exchange of both parts with the z neighbours (two-pass schedule): H phase = top H_x, H_y planes
  // up, E phase = bottom E_x, E_y planes down; a plane that crossed the periodic wrap is rotated where it lands
  int exchange_pair(bool e_side) {
    const int c0 = e_side ? 0 : 3;
    NCCLCHK(hr, ncclGroupStart());
    for (FdtdSolver* h : both)
      for (int c = c0; c < c0 + 2; ++c) {
        float* f = field_ptr(h, c);
        if (!e_side && nb_hi) NCCLCHK(hr, ncclSend(f + (long long)(nz - 1) * pc, pc, ncclFloat, hi_rank, hr->comm, st));
        if (e_side && nb_lo) NCCLCHK(hr, ncclSend(f, pc, ncclFloat, lo_rank, hr->comm, st));
      }
    for (FdtdSolver* h : both)
      for (int c = c0; c < c0 + 2; ++c) {
        float* f = field_ptr(h, c);
        if (!e_side && nb_lo) NCCLCHK(hr, ncclRecv(f - pc, pc, ncclFloat, lo_rank, hr->comm, st));
        if (e_side && nb_hi) NCCLCHK(hr, ncclRecv(f + (long long)nz * pc, pc, ncclFloat, hi_rank, hr->comm, st));
      }
    NCCLCHK(hr, ncclGroupEnd());
    if (!e_side && wrap_lo) { plane(3, -1, -1, -sph[2]); plane(4, -1, -1, -sph[2]); }       // exp(-i phi_z), in place
    if (e_side && wrap_hi) { plane(0, nz, nz, sph[2]); plane(1, nz, nz, sph[2]); }          // exp(+i phi_z)
    return 0;
  }
  // the E-side terms of step n behind the update of both parts.  With coupling lists: the head of both parts, the coupling (it reads
  // both parts), the tail of both; without, the parts are independent and each takes the whole.  (all planes; a z-slab rank — not the
  // whole grid — carries no whole-grid lists: setup)
  void e_terms(long long n) {
    if (!aniso) { for (FdtdSolver* h : both) e_side_terms(h, n, 0, nz, st, !multi); return; }
    for (FdtdSolver* h : both) e_side_head(h, n, 0, nz, st);
    aniso_apply_bloch(hr, hi, wrap_tab, st);
    for (FdtdSolver* h : both) e_side_tail(h, n, 0, nz, st, !multi);
  }
  // one step of both parts
  int step() {
    const long long n = hr->step;
    const bool rec = rec_at(hr, n);
    if (rec) for (FdtdSolver* h : both) record_monitors(h, n, false, st);
    if (aniso) aniso_save_bloch(hr, hi, st);     // (E^n of the nodes around fully anisotropic cells, in front of either sweep)
    for (FdtdSolver* h : both) modulation_save(h, st);      // (E^n of the nodes inside time-modulated media, likewise)
    // H-side corrections of both parts, then the ghost cells (they must carry the corrections too)
    for (FdtdSolver* h : both) h_side_terms(h, n, 0, nz, st);
    fill_xy();
    if (fused) {
      if (per_z) {       // ghost(-1) = exp(-i phi_z) [E (3 comps), H_x, H_y][nz-1];  ghost(nz) = exp(+i phi_z) E_{x,y}[0]
        for (int c = 0; c < 5; ++c) plane(c, -1, nz - 1, -sph[2]);
        plane(0, nz, 0, sph[2]);
        plane(1, nz, 0, sph[2]);
      }
      for (FdtdSolver* h : both) if (launch_fused(h, st, 0)) return -1;
      if (rec) for (FdtdSolver* h : both) record_monitors(h, n, true, st);
      e_terms(n);
    } else {
      if (per_z) { plane(0, nz, 0, sph[2]); plane(1, nz, 0, sph[2]); }      // E ghost(nz) of E^n (first step / after set_field)
      if (multi && exchange_pair(true)) return -1;                          // ... or the upper neighbour's bottom plane
      for (FdtdSolver* h : both) launch_h_main(h, 0, nz, st);
      if (per_z) { plane(3, -1, nz - 1, -sph[2]); plane(4, -1, nz - 1, -sph[2]); }
      else if (!nb_lo) for (FdtdSolver* h : both) fill_ghost_h(h, st);
      if (multi && exchange_pair(false)) return -1;
      if (rec) for (FdtdSolver* h : both) record_monitors(h, n, true, st);
      for (FdtdSolver* h : both) launch_e_main(h, 0, nz, st);
      e_terms(n);
      if (!per_z && !nb_hi) for (FdtdSolver* h : both) fill_ghost_e(h, st);
    }
    hr->step = hi->step = n + 1;
    return 0;
  }
  // field decay / divergence (|E|^2 of both parts) every decay_every steps.  -> 1: the run ends here
  int decay_check() {
    if (!(hr->decay_every > 0 && (hr->step % hr->decay_every) == 0)) return 0;
    double en = 0.0;
    for (FdtdSolver* h : both) {
      double part = 0.0;
      if (eval_energy(h, st, &part)) { hr->err = h->err; return -1; }
      en += part;
    }
    if (multi && allreduce_energy(hr, &en, st)) return -1;      // (the same stream as every other RCCL call of this run)
    return decay_verdict({hr, hi}, en, progress, user);
  }
  int loop() {
    for (int64_t done = 0; done < n_steps; ++done) {
      if (step()) return -1;
      const int dc = decay_check();
      if (dc < 0) return -1;
      if (dc > 0) break;
    }
    return 0;
  }
  int finish() {
    fill_xy();                   // leave the ghost cells of E^n, H^{n-1/2} consistent for whoever reads the fields next
    HIPCHK(hr, hipEventRecord(hr->ev1, st));
    HIPCHK(hr, hipStreamSynchronize(st));
    HIPCHK(hr, hipGetLastError());
    return run_stats({hr, hi});
  }
};
