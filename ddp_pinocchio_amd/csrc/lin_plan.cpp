// lin_plan.cpp -- which kernels a context's linearisation runs: one pure function, no HIP calls, and the
// development switches it is a function of, read from the environment.
// With -DLIN_PLAN_TABLE the file is a program that prints the plan of every combination of its inputs (tests/test_lin_plan.py),
// or, as `lin_plan_table schedule` / `lin_plan_table caches` / `lin_plan_table vcaches`, the schedule / the cache layouts of the flagship plan under the
// environment's switches (tests/test_lin_overlap.py, tests/test_sparse_caches.py, tests/test_sparse_vcache.py).
#include <stdlib.h>

#include "internal.h"

// The development switches: the one place in the library that reads the environment
DevSwitches read_switches() {
  auto on = [](const char* name) { return getenv(name) != nullptr; };
  auto knob = [](const char* name, int lo, int hi) { const char* ev = getenv(name); const int v = ev ? atoi(ev) : 0; return v >= lo && v <= hi ? v : 0; };
  DevSwitches sw;
  sw.generic_bwd = on("DDP_HIP_GENERIC_BWD");
  sw.k3_no_sym = on("DDP_HIP_K3_NO_SYM");
  sw.k3_no_half = on("DDP_HIP_K3_NO_HALF");
  sw.k3_no_pack = on("DDP_HIP_K3_NO_PACK");
  sw.k3h_column_jobs = on("DDP_HIP_K3H_COLUMN_JOBS");
  sw.fxx_full = on("DDP_HIP_FXX_FULL");
  sw.no_static = on("DDP_HIP_NO_STATIC");
  sw.no_qcache = on("DDP_HIP_NO_QCACHE");
  sw.qcache_dense = on("DDP_HIP_QCACHE_DENSE");
  sw.vcache_dense = on("DDP_HIP_VCACHE_DENSE");
  sw.first_scalar = on("DDP_HIP_FIRST_SCALAR");
  sw.cfg_full_aba = on("DDP_HIP_CFG_FULL_ABA");
  sw.ana_own_aba = on("DDP_HIP_ANA_OWN_ABA");
  sw.ana_split = on("DDP_HIP_ANA_SPLIT");
  sw.ana_eq_kernel = on("DDP_HIP_ANA_EQ_KERNEL");
  sw.bwd_no_graph = on("DDP_HIP_BWD_NO_GRAPH");
  sw.solve_sync = on("DDP_HIP_SOLVE_SYNC");
  sw.fwd_no_pipe = on("DDP_HIP_FWD_NO_PIPE");
  sw.lin_serial = on("DDP_HIP_LIN_SERIAL");
  sw.lin_forks = knob("DDP_HIP_LIN_FORKS", 1, 3);
  sw.bwd_cbx = knob("DDP_HIP_BWD_CBX", 1, 8);
  sw.bwd_cbu = knob("DDP_HIP_BWD_CBU", 1, 16);
  sw.qws_bt = knob("DDP_HIP_QWS_BT", 16, 65536);
  sw.ana_bt = knob("DDP_HIP_ANA_BT", 1, 65536);
  return sw;
}

// topo_id: what lin_static_supported returned for the model's tree (0: no compiled-in topology, always 0 with a free flyer);
// sweep_sym_ok: sweep_plan(ctx).sym_ok, a property of the shape and the switches alone (bwd_setup runs ahead of lin_setup)
LinPlan lin_plan_decide(const DevModel& m, const Dims& d, uint32_t flags, const DevSwitches& sw, int topo_id, bool sweep_sym_ok) {
  LinPlan pl;
  const bool tree = m.kind == DDP_HIP_MODEL_TREE, ff = m.ff != 0, fo_fd = m.first_order_fd != 0;
  const bool tensors = !(flags & DDP_HIP_FLAG_NO_TENSORS);
  const bool analytic = tree && !fo_fd;
  const int mode = m.fd_mode;
  const int64_t nv = d.nv, K = m.eq_advance;
  pl.has_tensors = tensors;
  pl.nj = nv <= 1 ? 1 : (nv <= 6 && !ff) ? 6 : nv <= 38 ? 38 : 64;   // (the one-lane kernels of small models are vector-space only)
  const bool small = pl.nj <= 6;
  const bool wave = analytic && !small && !ff;   // lin_analytic.hip's wave kernels: large trees of 1-DoF joints

  // forward differences of forward-differenced jacobians are numerically void -- eps_mach / sqrt(eps_mach)^2 = O(1) noise -- and the
  // reference cannot express them (its first order is always analytic)
  if (mode == 1 && fo_fd && tensors) pl.refuse = DDP_HIP_E_UNSUPPORTED;
  if (analytic && ff && nv > 38) pl.refuse = DDP_HIP_E_UNSUPPORTED;               // ana_ff_first_kernel<38>
  if (wave && m.max_level_width > 64) pl.refuse = DDP_HIP_E_UNSUPPORTED;           // a tree level per wave
  if (wave && d.Etot > 0 && (K < 1 || K > 2)) pl.refuse = DDP_HIP_E_UNSUPPORTED;   // ana_eq_kernel: K <= 2 look-ahead steps

  // the caches: the mode-2 stencil's (they index q by joint: trees of 1-DoF joints), or the base point alone for the static
  // first-order kernels -- forward-differenced jacobians, or the accelerations of analytic mode 1's perturbed points
  const int topo = (tree && !ff && !sw.no_static) ? topo_id : 0;
  const bool stencil_caches = tree && mode == 2 && tensors && !ff && !sw.no_qcache;
  const bool accel = topo && wave && mode == 1 && tensors && !sw.ana_own_aba;
  if (stencil_caches) { pl.ncfg = (int32_t)nv + 1; pl.nvcfg = 2 * (int32_t)nv + 1; }
  else if ((topo && fo_fd) || accel) { pl.ncfg = 1; pl.nvcfg = 1; }
  pl.ws_lin = pl.ncfg > 0;
  pl.topo = pl.ws_lin ? topo : 0;   // without caches nothing runs on the static kernels
  pl.ws_qws = pl.topo != 0;

  if (analytic) pl.first = small ? LinFirst::AnalyticSmall : ff ? LinFirst::AnalyticFF : LinFirst::AnalyticWave;
  else if (fo_fd) pl.first = pl.topo ? LinFirst::FdStatic : LinFirst::FdGeneric;
  else pl.first = LinFirst::Base;

  if (!tensors) pl.second = LinSecond::None;
  else if (mode == 0) pl.second = LinSecond::Zeros;
  else if (mode == 1) pl.second = small ? LinSecond::Mode1Small : LinSecond::Mode1Wave;
  else if (pl.ncfg > 1) pl.second = pl.topo ? LinSecond::Mode2Static : LinSecond::Mode2Caches;
  else pl.second = LinSecond::Mode2Plain;
  pl.ws_qws2 = pl.second == LinSecond::Mode2Static && sw.cfg_full_aba;
  // base + deltas q-cache: the static stencil's readers alone know it (the full-ABA configuration level reads whole blocks)
  pl.qc_sparse = pl.second == LinSecond::Mode2Static && !sw.qcache_dense && !sw.cfg_full_aba;
  pl.vc_sparse = pl.qc_sparse && !sw.vcache_dense;
  // (with DDP_HIP_NO_QCACHE on forward-differenced jacobians the two marks below are set although Mode2Plain runs: DESIGN.md 4j)
  pl.skip_top = pl.topo && mode == 2 && tensors && !sw.fxx_full;
  pl.skip_qv_mirror = pl.skip_top && sweep_sym_ok;   // only for a sweep that never reads the mirror images
  // packed records: the static stencil writing for the fast symmetric sweep's K3h (sweep_sym_ok: the Talos shape, where K3h's job list exists)
  pl.pack = pl.skip_qv_mirror && pl.second == LinSecond::Mode2Static && !sw.k3_no_half && !sw.k3_no_pack;

  const bool m1_wave = wave && pl.second == LinSecond::Mode1Wave;
  pl.ana_sliced = analytic && !small;
  pl.ws_ana_T = wave && sw.ana_split;
  pl.ws_ana_M = wave && (sw.ana_split || (m1_wave && d.Etot > 0));
  pl.ws_ana_M0 = m1_wave && !sw.ana_split;
  pl.ws_ana_A = pl.accel_static = accel;
  pl.accel_with_u = accel && d.Etot > 0;
  pl.ws_ana_F = m1_wave && d.Etot > 0;

  pl.ws_eq = d.Etot > 0 && tree && (fo_fd || ff);
  if (d.Etot > 0) {
    pl.eq = (small && !pl.ws_eq) ? LinEq::PerLane : wave ? LinEq::Analytic : LinEq::Chain;
    if (pl.eq == LinEq::Chain && K > 1) pl.eq_jac = fo_fd ? LinEqJac::Fd : LinEqJac::FfLookahead;
    pl.eq_second = !tensors ? LinEqSecond::None : mode == 0 ? LinEqSecond::Zeros : mode == 2 ? LinEqSecond::Mode2
                   : small ? LinEqSecond::Mode1Small : LinEqSecond::Mode1Wave;
    pl.m1_fused = m1_wave;
    pl.eq_inline = m1_wave && !sw.ana_split && m.eq_kind == DDP_HIP_EQ_CONFIG && !sw.ana_eq_kernel;
  }
  if (pl.ws_eq) {
    pl.eq_fxk_off = d.batch * d.T * K * d.nx;
    pl.eq_c_off = pl.eq_fxk_off + d.batch * d.T * (K > 1 ? K - 1 : 0) * d.n * d.n;
    pl.eq_words = pl.eq_c_off + d.batch * d.T * d.emax * d.n;
  }
  // the concurrent schedule: the static stencil's own.  The full-ABA configuration level keeps its two-stream
  // slice pipeline to itself
  if (pl.second == LinSecond::Mode2Static && !sw.lin_serial && !sw.cfg_full_aba) pl.forks = sw.lin_forks ? (uint32_t)sw.lin_forks : (uint32_t)LIN_FORK_DEFAULT;
  pl.lin_path = tree ? 1 + pl.topo : 0;
  pl.first_order = tree ? (fo_fd ? 1 : 2) : 0;
  return pl;
}

#ifdef LIN_PLAN_TABLE
#include <stdio.h>

// One line of integers per combination of the inputs (the first line names the columns).  `created`: ddp_hip_create's own
// argument checks let the combination through to lin_setup (ctx.hip: a pendulum has nv = 1 and no free flyer; a free flyer
// leaves nj = nv - 5 >= 1 joints and is refused in mode 1 and under the config constraint; no constraint kind, no rows).
int main(int argc, char** argv) {
  if (argc > 1 && (argv[1][0] == 's' || argv[1][0] == 'c' || argv[1][0] == 'v')) {
    // `schedule`: the forks of the flagship plan (Talos-size tree on its compiled-in topology, mode 2, forward-differenced first
    // order) under the switches of this process's environment (tests/test_lin_overlap.py)
    DevModel m{};
    m.kind = DDP_HIP_MODEL_TREE; m.nv = 38; m.nj = 38; m.nq = 38; m.first_order_fd = 1; m.fd_mode = 2; m.max_level_width = 4;
    Dims d{};
    d.T = 3; d.batch = 2; d.nv = 38; d.n = 76; d.m = 38; d.nx = 76;
    const LinPlan p = lin_plan_decide(m, d, 0u, read_switches(), 1, true);
    // `caches`: the q-cache layout of the same plan (tests/test_sparse_caches.py)
    if (argv[1][0] == 'c') { printf("qc_sparse %d ncfg %d nvcfg %d\n", (int)p.qc_sparse, p.ncfg, p.nvcfg); return 0; }
    // `vcaches`: its v-cache layout (tests/test_sparse_vcache.py)
    if (argv[1][0] == 'v') { printf("vc_sparse %d qc_sparse %d nvcfg %d\n", (int)p.vc_sparse, (int)p.qc_sparse, p.nvcfg); return 0; }
    printf("forks %u topo %d\n", p.forks, p.topo);
    return 0;
  }
  static const char* const sw_names[] = {"none", "generic_bwd", "k3_no_sym", "k3_no_half", "fxx_full", "no_static", "no_qcache",
                                         "cfg_full_aba", "ana_own_aba", "ana_split", "ana_eq_kernel", "bwd_no_graph", "solve_sync"};
  printf("kind nv ff fo_fd mode tensors etot eq_kind K matched sw sym_ok created refuse nj topo first second eq eq_jac eq_second "
         "eq_inline accel_static accel_with_u m1_fused ncfg nvcfg has_tensors skip_top skip_qv_mirror pack ws_lin ws_qws ws_qws2 ws_ana_T "
         "ws_ana_M ws_ana_M0 ws_ana_A ws_ana_F ws_eq ana_sliced eq_fxk_off eq_c_off eq_words lin_path first_order\n");
  printf("#");
  for (const char* s : sw_names) printf(" %s", s);
  printf("\n");
  const int nvs[] = {1, 6, 7, 38, 39, 64};
  for (int kind : {DDP_HIP_MODEL_PENDULUM, DDP_HIP_MODEL_TREE})
  for (int nv : nvs) for (int ff = 0; ff < 2; ++ff) for (int fo = 0; fo < 2; ++fo) for (int mode = 0; mode < 3; ++mode)
  for (int tensors = 0; tensors < 2; ++tensors) for (int etot = 0; etot < 2; ++etot)
  for (int eqk : {DDP_HIP_EQ_NONE, DDP_HIP_EQ_CONFIG, DDP_HIP_EQ_FRAME}) for (int K = 1; K <= 3; ++K)
  for (int matched = 0; matched < 2; ++matched) for (int s = 0; s < 13; ++s) {
    DevModel m{};
    m.kind = kind; m.nv = nv; m.ff = ff; m.nj = ff ? nv - 5 : nv; m.nq = nv + ff;
    m.first_order_fd = fo; m.fd_mode = mode; m.eq_kind = eqk; m.eq_advance = K; m.max_level_width = 4;
    Dims d{};
    d.T = 3; d.batch = 2; d.nv = nv; d.n = 2 * nv; d.m = nv; d.nx = 2 * nv + ff;
    d.emax = etot ? (eqk == DDP_HIP_EQ_CONFIG ? nv : 3) : 0; d.Etot = etot ? d.emax * d.T : 0;
    DevSwitches sw;
    bool* const sws[] = {nullptr, &sw.generic_bwd, &sw.k3_no_sym, &sw.k3_no_half, &sw.fxx_full, &sw.no_static, &sw.no_qcache,
                         &sw.cfg_full_aba, &sw.ana_own_aba, &sw.ana_split, &sw.ana_eq_kernel, &sw.bwd_no_graph, &sw.solve_sync};
    if (sws[s]) *sws[s] = true;
    const int sym_ok = nv == 38 && !sw.generic_bwd && !sw.k3_no_sym;   // bwd.hip: sweep_plan (d.emax <= 52 here)
    const bool created = (kind == DDP_HIP_MODEL_TREE || (nv == 1 && !ff)) && (!ff || (nv >= 6 && mode != 1 && eqk != DDP_HIP_EQ_CONFIG)) &&
                         (eqk != DDP_HIP_EQ_NONE || !etot);
    const LinPlan p = lin_plan_decide(m, d, tensors ? 0u : (uint32_t)DDP_HIP_FLAG_NO_TENSORS, sw, matched && !ff ? 1 : 0, sym_ok != 0);
    printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %lld %lld %lld %d %d\n",
           kind == DDP_HIP_MODEL_TREE, nv, ff, fo, mode, tensors, etot, eqk == DDP_HIP_EQ_NONE ? 0 : eqk == DDP_HIP_EQ_CONFIG ? 1 : 2, K, matched, s, sym_ok,
           (int)created, p.refuse != 0, p.nj, p.topo, (int)p.first, (int)p.second, (int)p.eq, (int)p.eq_jac, (int)p.eq_second,
           (int)p.eq_inline, (int)p.accel_static, (int)p.accel_with_u, (int)p.m1_fused, p.ncfg, p.nvcfg, (int)p.has_tensors, (int)p.skip_top,
           (int)p.skip_qv_mirror, (int)p.pack, (int)p.ws_lin, (int)p.ws_qws, (int)p.ws_qws2, (int)p.ws_ana_T, (int)p.ws_ana_M, (int)p.ws_ana_M0, (int)p.ws_ana_A,
           (int)p.ws_ana_F, (int)p.ws_eq, (int)p.ana_sliced, (long long)p.eq_fxk_off, (long long)p.eq_c_off, (long long)p.eq_words, p.lin_path, p.first_order);
  }
  return 0;
}
#endif
