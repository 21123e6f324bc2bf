// bwd_split.h -- the tensor stream of the Talos-shape backward step (included by bwd.hip before bwd_v2.h):
//
//   K3  bwd_contract<N, M>   grid (jobs, batch).  Pure HBM stream: C(j,k) = sum_i V_x,i T(i,j,k) for the three
//       second-order tensors of one timestep (tensor.hpp:179-198 as called at ddp_bwd.ipp:75,81,87).
//       Reads every tensor byte exactly once with 16-byte coalesced loads, three 69 KB units per workgroup
//       always in flight; 0.25 flop/byte.
//   K3h bwd_contract_half<N, M>  the same contraction for tensors with known structure: reads only what is not known
//       in advance (below).
//   K3h on full units  bwd_contract_units<N, M, UPJ>  K3h for the stencil's packed records, on a job list without empty
//       column slots (bwd_jobs.h; at the end of this file).
//   All add C to the Q workspace, which already holds every other term of Q (K5, bwd_v2.h).
#pragma once

template <int N, int M>
__global__ __launch_bounds__(BSF, BWD_WAVES_PER_SIMD) void bwd_contract(BwdParams p, int64_t t) {
  // XCD-aware placement: blocks b and b+8 share an XCD; keep the jobs of one instance on one XCD (speed only)
  int b, jb;
  {
    const int njobs = (int)gridDim.x, B = (int)gridDim.y;
    const int lin = blockIdx.y * njobs + blockIdx.x;
    if ((B & 7) == 0) {
      const int xcd = lin & 7, k = lin >> 3;
      b = xcd + 8 * (k / njobs);
      jb = k % njobs;
    } else { b = blockIdx.y; jb = blockIdx.x; }
  }
  if (p.status[b] != 0) return;
  const BwdJob job = p.jobs[jb];
  constexpr int n = N, m = M;
  const int64_t T = p.d.T;
  const int tid = threadIdx.x;
  // kind 0: x-columns (f_xx in two half-slabs, f_ux), 1: u-columns (f_uu), 2: x-columns c >= M without their first half-slab.
  // SYMMETRIC tensors (p.sym_tensors: this context's own mode-2 or zero tensors -- the stencil forms one value for the entries
  // (i, j, c) and (i, c, j), problem.hpp:283-292): of slab c only the columns j >= c are read -- one contiguous tail of the slab
  // -- and the contraction C(j, c) is written to (j, c) and to its mirror image (c, j); the entries j < c come from the jobs of
  // the columns j.  The mirrored sum is the very sum the skipped column would have given, bit for bit.  Half of f_xx and of
  // f_uu (2.16 of 6.31 MB per (instance, t)) is never read, and the stencil does not have to write it (lin_static.hip)
  const int kind = job.kind, c0 = job.c0, cn = job.cn;
  const int rows = kind == 1 ? m : n + m;
  static_assert(N == 2 * M, "half-slabs: the state tangent is twice the control dimension");
  const int64_t bt = (int64_t)b * T + t;

  const double* Vx = p.ws_V + (int64_t)b * (n + n * n);
  double* C = p.ws_Q + (int64_t)b * (n + m + n * n + m * n + m * m) + n + m;   // Q_xx | Q_ux | Q_uu, holding what K5 left
  double* Cxx = C;
  double* Cux = Cxx + n * n;
  double* Cuu = Cux + m * n;

  using US = SlabShape<N, M>;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* s_v = smem;                          // n
  double* s_out = s_v + n;                     // rows * cn
  double* s_p0 = s_out + (n + m) * cn;         // US::LD * M
  double* s_p1 = s_p0 + US::LD * M;

  // units: 76 x 38 column-major blocks; an x-column is f_xx(:,0:38,c), f_xx(:,38:76,c), f_ux(:,:,c); a u-column f_uu(:,:,c)
  const int upc = kind == 0 ? 3 : (kind == 2 ? 2 : 1);
  const int part0 = kind == 2 ? 1 : 0;              // first part (row block of the column) this job reads
  const int U = upc * cn;
  const double* Txx = p.fxx + (bt * n + c0) * (int64_t)n * n;
  const double* Tux = p.fux + (bt * n + c0) * (int64_t)n * m;
  const double* Tuu = p.fuu + (bt * m + c0) * (int64_t)n * m;
  auto unit_ptr = [&](int u) -> const double* {
    const int c = u / upc, part = u - c * upc + part0;
    if (kind != 1) return part < 2 ? Txx + (int64_t)c * n * n + part * (M * n) : Tux + (int64_t)c * n * m;
    return Tuu + (int64_t)c * n * m;
  };
  const bool sym = p.sym_tensors != 0;
  auto unit_jmin = [&](int u) -> int {                 // first column of the unit that is read
    if (!sym) return 0;
    const int c = u / upc, part = u - c * upc + part0, col = c0 + c;
    if (kind == 1) return col;                        // f_uu(:, j, col): j >= col
    if (part == 0) return col < M ? col : M;          // f_xx(:, 0:M, col)
    if (part == 1) return col > M ? col - M : 0;      // f_xx(:, M:N, col)
    return 0;                                         // f_ux
  };
  f64x2 buf0[US::R], buf1[US::R], buf2[US::R], buf3[US::R];
#define C_ISSUE(BUF, u) do { if ((u) < U) slab_issue_from<N, M, BWD_NT>(unit_ptr(u), BUF, unit_jmin(u)); } while (0)
  C_ISSUE(buf0, 0); C_ISSUE(buf1, 1); C_ISSUE(buf2, 2); C_ISSUE(buf3, 3);

  for (int i = tid; i < n; i += BSF) s_v[i] = Vx[i];
  for (int i = tid; i < rows * cn; i += BSF) s_out[i] = 0.0;
  __syncthreads();

#define C_STEP(BUF, u)                                                                      \
  do {                                                                                      \
    if ((u) < U) {                                                                          \
      double* sp = ((u) & 1) ? s_p1 : s_p0;                                                 \
      _Pragma("unroll") for (int r = 0; r < US::R; ++r) {                                   \
        const int f = tid + r * BSF;                                                        \
        if (r < US::R - 1 || f < US::TOTAL) {                                               \
          const int j = f / US::HP;                                                         \
          const int ip = f - j * US::HP;                                                    \
          const f64x2 vv = *reinterpret_cast<const f64x2*>(s_v + 2 * ip);                   \
          sp[j * US::LD + ip] = vv.x * BUF[r].x + vv.y * BUF[r].y;                          \
        }                                                                                   \
      }                                                                                     \
      __syncthreads();                                                                      \
      if (tid < M) {                                                                        \
        const double* pj = sp + tid * US::LD;                                               \
        double sacc = 0.0;                                                                  \
        _Pragma("unroll") for (int k = 0; k < US::HP; ++k) sacc += pj[k];                   \
        const int c_ = (u) / upc, part_ = (u) - c_ * upc + part0;                           \
        s_out[c_ * rows + part_ * M + tid] = sacc;                                          \
      }                                                                                     \
      C_ISSUE(BUF, (u) + 4);                                                                \
    }                                                                                       \
  } while (0)
  for (int u = 0; u < U; u += 4) {
    C_STEP(buf0, u);
    C_STEP(buf1, u + 1);
    C_STEP(buf2, u + 2);
    C_STEP(buf3, u + 3);
  }
  __syncthreads();
#undef C_STEP
#undef C_ISSUE
  for (int idx = tid; idx < rows * cn; idx += BSF) {
    const int r = idx % rows, c = idx / rows;
    const int col = c0 + c;
    // the workspace already holds every other term of Q (K5, bwd_v2.h); the tensor term comes last in the reference as well
    // (ddp_bwd.ipp:75,81,87)
    if (kind == 2 && r < M) continue;                // (the half-slab this job kind leaves out)
    const bool square = kind == 1 || r < n;          // an entry of C_xx / C_uu (f_ux is not symmetric)
    if (sym && square && r < col) continue;          // the mirror image: written by the job of column r
    double* dst = kind != 1 ? (r < n ? Cxx + r + col * n : Cux + (r - n) + col * m) : Cuu + r + col * m;
    *dst = *dst + s_out[idx];
    if (sym && square && r > col) {
      double* dm = kind != 1 ? Cxx + col + r * n : Cuu + col + r * m;   // C(col, r) = C(r, col)
      *dm = *dm + s_out[idx];
    }
  }
}

// ---- K3h: the same contraction for this context's own mode-2 tensors, reading what is not known in advance ------------------
// Two structural facts about the tensors the stencil (lin_static.hip / lin.hip) writes, both exact in floating point:
//  (1) symmetry: entries (i, j, c) and (i, c, j) of f_xx / f_uu hold one value (problem.hpp:283-292) -> of slab c only the
//      columns j >= c are read, the contraction goes to (j, c) and to (c, j);
//  (2) the CONFIGURATION rows i < M of every column are exact zeros except at i = c mod M and i = j mod M (x directions): the
//      first M rows of f are q + dt v, which does not see the dynamics, so row i of a stencil point differs from the base
//      point's only when a direction is q_i or v_i; everything else differences bit-identical numbers.
// So a column contributes  sum_{i >= M} V_x,i T(i, j, c)  plus at most two terms from its first M rows.  A unit is the lower
// half (rows M .. N-1: 304 contiguous bytes per column) of N consecutive columns -- one slab of f_xx, two of f_ux or f_uu -- as
// many bytes as bwd_contract's unit; the (at most) two entries of the upper half come with two 8-byte loads per column.  The sums
// are formed in bwd_contract's order -- two-term partials over the row pairs (2 ip, 2 ip + 1), then ip ascending, the zero
// partials adding nothing -- so the result is bwd_contract's bit for bit (tests/test_round3_boundary.py).
// Bytes per (instance, t): 2.08 MB of lower halves + 0.13 MB of single entries against 6.31 MB (SURVEY.md 8d's formula).
template <int N, int M>
struct HalfShape {
  static constexpr int HP = M / 2, LD = M / 2 + 1, TOTAL = (M / 2) * N, R = ((M / 2) * N + BSF - 1) / BSF;   // f64x2 words of a unit
};
static_assert(38 % 2 == 0, "row pairs");

// kinds: 10 = x-columns c0, c0 + 1 (units: f_xx slab c0 | f_xx slab c0 + 1 | f_ux slabs c0, c0 + 1); 11 = cn u-columns from c0,
// cn even (units: f_uu slabs in pairs)
// PK: the tensors are the stencil's packed records (lin_common.h: LinParams::pack) -- column j of a slab is the M + 2 doubles
// [top0, top1, rows M .. N-1] at slab + j (M + 2), so a unit's bytes are one contiguous run per slab (two for f_ux / f_uu units,
// whose slabs keep their bases) and the two upper-half entries are word 0 of the record.  Same jobs, same lanes, same sums.
template <int N, int M, bool PK>
__global__ __launch_bounds__(BSF, BWD_WAVES_PER_SIMD) void bwd_contract_half(BwdParams p, int64_t t) {
  int b, jb;
  {
    const int njobs = (int)gridDim.x, B = (int)gridDim.y;
    const int lin = blockIdx.y * njobs + blockIdx.x;
    if ((B & 7) == 0) {
      const int xcd = lin & 7, k = lin >> 3;
      b = xcd + 8 * (k / njobs);
      jb = k % njobs;
    } else { b = blockIdx.y; jb = blockIdx.x; }
  }
  if (p.status[b] != 0) return;
  const BwdJob job = p.jobs_half[jb];
  constexpr int n = N, m = M;
  static_assert(N == 2 * M && M % 2 == 0, "lower halves of M rows, in row pairs");
  const int64_t T = p.d.T;
  const int tid = threadIdx.x;
  const int kind = job.kind, c0 = job.c0, cn = job.cn;
  const bool m1 = p.half_mode == 2;            // analytic mode-1 tensors: every column read, no upper-half entries, f_uu all zeros
  const int64_t bt = (int64_t)b * T + t;
  const double* Vx = p.ws_V + (int64_t)b * (n + n * n);
  double* C = p.ws_Q + (int64_t)b * (n + m + n * n + m * n + m * m) + n + m;   // Q_xx | Q_ux | Q_uu, holding what K5 left
  double* Cxx = C;
  double* Cux = Cxx + n * n;
  double* Cuu = Cux + m * n;
  using HS = HalfShape<N, M>;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* s_v = smem;                          // n
  double* s_out = s_v + n;                     // units x N
  double* s_p0 = s_out + 3 * N;                // HS::LD * N
  double* s_p1 = s_p0 + HS::LD * N;
  const int U = kind == 10 ? 3 : cn / 2;
  // unit u: its N columns are slab / column pairs (sl, j): which tensor, which slab, the direction index of the column
  auto unit_base = [&](int u) -> const double* {
    if (kind == 10) return u < 2 ? p.fxx + (bt * n + c0 + u) * (int64_t)n * n : p.fux + (bt * n + c0) * (int64_t)n * m;
    return p.fuu + (bt * m + c0 + 2 * u) * (int64_t)n * m;
  };
  // column jj of unit u: slab index (the first direction of the pair), column index within its tensor, and whether the column is
  // read at all (symmetric tensors: j >= slab)
  auto col_info = [&](int u, int jj, int& slab, int& j, bool& xcol) -> bool {
    if (kind == 10) {
      if (u < 2) { slab = c0 + u; j = jj; xcol = true; return m1 || j >= slab; }          // f_xx(:, j, slab)
      slab = c0 + (jj >= m ? 1 : 0); j = jj >= m ? jj - m : jj; xcol = false; return true;   // f_ux(:, j, slab)
    }
    slab = c0 + 2 * u + (jj >= m ? 1 : 0); j = jj >= m ? jj - m : jj; xcol = false; return m1 || j >= slab;   // f_uu(:, j, slab)
  };
  f64x2 buf0[HS::R], buf1[HS::R], buf2[HS::R], buf3[HS::R];
  double top0[2], top1[2], top2[2], top3[2];   // lane jj < N: the (at most) two entries of its column's upper half
  auto issue = [&](int u, f64x2 (&buf)[HS::R], double (&top)[2]) {
    const f64x2* base = reinterpret_cast<const f64x2*>(unit_base(u));
    // packed: first word of column jj's record (a unit of two M-column slabs: the second slab's records start at its own base)
    const bool two = !(kind == 10 && u < 2);
    auto rec_word = [&](int jj) -> int { return (two && jj >= m) ? (N * M) / 2 + (jj - m) * (HS::HP + 1) : jj * (HS::HP + 1); };
#pragma unroll
    for (int r = 0; r < HS::R; ++r) {
      const int f = tid + r * BSF;
      bool need = r < HS::R - 1 || f < HS::TOTAL;
      const int jj = f / HS::HP, ip = f - jj * HS::HP;
      int slab, j; bool xcol;
      if (need) need = col_info(u, jj < n ? jj : n - 1, slab, j, xcol) && !(m1 && kind == 11);
      const int w = PK ? rec_word(jj) + 1 + ip : jj * (N / 2) + HS::HP + ip;
      if (need) buf[r] = BWD_NT ? __builtin_nontemporal_load(&base[w]) : base[w];
      else buf[r] = f64x2{0.0, 0.0};
    }
    top[0] = 0.0; top[1] = 0.0;
    if (tid < n) {
      int slab, j; bool xcol;
      if (col_info(u, tid, slab, j, xcol) && kind == 10 && !m1) {   // f_uu: its directions are controls, the upper half is all zeros
        if constexpr (PK) {
          const f64x2 tw = base[rec_word(tid)];
          top[0] = tw.x;
          if (xcol && (j % M) != (slab % M)) top[1] = tw.y;          // (else: never written)
        } else {
          const double* colp = unit_base(u) + (int64_t)tid * n;
          top[0] = colp[slab % M];                                     // the slab's direction is an x direction (f_xx and f_ux)
          if (xcol && (j % M) != (slab % M)) top[1] = colp[j % M];
        }
      }
    }
  };
  if (U > 0) issue(0, buf0, top0);
  if (U > 1) issue(1, buf1, top1);
  if (U > 2) issue(2, buf2, top2);
  // this lane's output entry (U * N <= BSF: one per lane) and what the workspace holds there (the dense terms K5 left),
  // requested now so that the read-modify-write at the end does not wait for a round trip of its own
  double* dst = nullptr;
  double* dm = nullptr;
  double old_d = 0.0, old_m = 0.0;
  static_assert(3 * N <= BSF, "one output entry per lane");
  if (tid < U * N) {
    const int u = tid / N, jj = tid - u * N;
    int slab, j; bool xcol;
    if (col_info(u, jj, slab, j, xcol)) {                  // (else: the mirror image, written by the job of the other column)
      if (kind == 10) {
        if (u < 2) { dst = Cxx + j + slab * n; if (j > slab && !m1) dm = Cxx + slab + j * n; }
        else dst = Cux + j + slab * m;
      } else { dst = Cuu + j + slab * m; if (j > slab && !m1) dm = Cuu + slab + j * m; }
      old_d = *dst;
      if (dm) old_m = *dm;
    }
  }
  for (int i = tid; i < n; i += BSF) s_v[i] = Vx[i];
  __syncthreads();
  auto step = [&](int u, f64x2 (&buf)[HS::R], double (&top)[2]) {
    double* sp = (u & 1) ? s_p1 : s_p0;
#pragma unroll
    for (int r = 0; r < HS::R; ++r) {
      const int f = tid + r * BSF;
      if (r < HS::R - 1 || f < HS::TOTAL) {
        const int jj = f / HS::HP, ip = f - jj * HS::HP;
        const f64x2 vv = *reinterpret_cast<const f64x2*>(s_v + M + 2 * ip);
        sp[jj * HS::LD + ip] = vv.x * buf[r].x + vv.y * buf[r].y;
      }
    }
    __syncthreads();
    if (tid < n) {
      int slab, j; bool xcol;
      const bool need = col_info(u, tid, slab, j, xcol);
      double sacc = 0.0;
      if (need && kind == 10 && !m1) {
        // the upper half's partials, in bwd_contract's order: row pair (2 ip, 2 ip + 1), ip ascending; all others are zeros
        const int ra = slab % M, rb = xcol ? j % M : ra;
        const int lo = ra < rb ? ra : rb, hi = ra < rb ? rb : ra;
        const double tlo = ra <= rb ? top[0] : top[1], thi = ra <= rb ? (ra == rb ? 0.0 : top[1]) : top[0];
        if (lo == hi) {
          const int e = lo & ~1;
          const f64x2 vv = *reinterpret_cast<const f64x2*>(s_v + e);
          const double tx = (lo & 1) ? 0.0 : tlo, ty = (lo & 1) ? tlo : 0.0;
          sacc += vv.x * tx + vv.y * ty;
        } else if ((lo >> 1) == (hi >> 1)) {
          const f64x2 vv = *reinterpret_cast<const f64x2*>(s_v + lo);      // lo even, hi = lo + 1
          sacc += vv.x * tlo + vv.y * thi;
        } else {
          const f64x2 va = *reinterpret_cast<const f64x2*>(s_v + (lo & ~1));
          const f64x2 vb = *reinterpret_cast<const f64x2*>(s_v + (hi & ~1));
          sacc += va.x * ((lo & 1) ? 0.0 : tlo) + va.y * ((lo & 1) ? tlo : 0.0);
          sacc += vb.x * ((hi & 1) ? 0.0 : thi) + vb.y * ((hi & 1) ? thi : 0.0);
        }
      }
      const double* pj = sp + tid * HS::LD;
#pragma unroll
      for (int k = 0; k < HS::HP; ++k) sacc += pj[k];
      s_out[u * N + tid] = sacc;
    }
  };
  // three units at most per job: all in flight from the start
  if (U > 0) step(0, buf0, top0);
  if (U > 1) step(1, buf1, top1);
  if (U > 2) step(2, buf2, top2);
  (void)buf3; (void)top3;
  __syncthreads();
  if (dst) {
    const double v = s_out[tid];
    *dst = old_d + v;
    if (dm) *dm = old_m + v;
  }
}

// ---- K3h on full units: the packed records of the symmetric tensors (half_mode 1), bwd_jobs.h's list ------------------------
// bwd_contract_half<N, M, true> gives every slab of f_xx / f_uu a unit of its own, and of slab c only the columns j >= c are
// needed: at (76, 38) 35 % of its column slots load nothing and still take their share of a barrier and a reduction.  Here a
// unit is a short list of RUNS -- cnt consecutive records of one slab -- whose columns fill the N slots one after another
// (bwd_jobs.h: k3h_full_units pairs the tails so that they do): 87 units instead of 133, 29 workgroups per instance instead of 45.
// A record is HP + 1 f64x2 words, [top0 top1 | rows M .. N-1], and a run is contiguous, so the lanes walk a unit word by word --
// (HP + 1) N <= R BSF words -- and the tops word comes with the same loads as the rows (it goes to the column's lane through LDS).
// The sums are bwd_contract_half's: a column's upper-half partials in bwd_contract's order, then its HP two-term partials with
// ip ascending, in one lane; which unit a column rides in changes nothing in them.  Every (tensor, slab, column) is in exactly
// one run (host/test_k3h_jobs.cpp), so one lane owns its entry of Q and the mirror entry.
template <int N, int M, int UPJ>
__global__ __launch_bounds__(BSF, BWD_WAVES_PER_SIMD) void bwd_contract_units(BwdParams p, int64_t t) {
  int b, jb;
  {
    const int njobs = (int)gridDim.x, B = (int)gridDim.y;
    const int lin = blockIdx.y * njobs + blockIdx.x;
    if ((B & 7) == 0) {
      const int xcd = lin & 7, k = lin >> 3;
      b = xcd + 8 * (k / njobs);
      jb = k % njobs;
    } else { b = blockIdx.y; jb = blockIdx.x; }
  }
  if (p.status[b] != 0) return;
  constexpr int n = N, m = M;
  static_assert(N == 2 * M && M % 2 == 0, "lower halves of M rows, in row pairs");
  using HS = HalfShape<N, M>;
  constexpr int W = HS::HP + 1;                      // f64x2 words of a record
  constexpr int R = (W * N + BSF - 1) / BSF;         // loads per lane and unit
  static_assert(UPJ * N <= BSF, "one output entry per lane");
  const K3hUnit* units = p.units_half + (int64_t)jb * UPJ;
  const int64_t T = p.d.T;
  const int tid = threadIdx.x;
  const int64_t bt = (int64_t)b * T + t;
  const double* Vx = p.ws_V + (int64_t)b * (n + n * n);
  double* C = p.ws_Q + (int64_t)b * (n + m + n * n + m * n + m * m) + n + m;   // Q_xx | Q_ux | Q_uu, holding what K5 left
  constexpr int OXX = 0, OUX = n * n, OUU = n * n + m * n;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* s_v = smem;                          // n
  double* s_out = s_v + n;                     // units x N
  double* s_p0 = s_out + UPJ * N;              // HS::LD * N
  double* s_p1 = s_p0 + HS::LD * N;
  f64x2* s_t0 = reinterpret_cast<f64x2*>(s_p1 + HS::LD * N);   // N tops words
  f64x2* s_t1 = s_t0 + N;
  // first word of a run's first record
  auto run_base = [&](const K3hRun& r) -> const f64x2* {
    const double* slab = r.tensor == K3H_FXX ? p.fxx + (bt * n + r.slab) * (int64_t)(n * n)
                       : r.tensor == K3H_FUX ? p.fux + (bt * n + r.slab) * (int64_t)(n * m)
                                             : p.fuu + (bt * m + r.slab) * (int64_t)(n * m);
    return reinterpret_cast<const f64x2*>(slab + (int64_t)r.j0 * (M + 2));
  };
  f64x2 buf[UPJ][R];
#pragma unroll
  for (int u = 0; u < UPJ; ++u) {
    const K3hUnit un = units[u];
    // word f of the unit is word f - e_k of run k
    const int e1 = W * un.run[0].cnt, e2 = e1 + W * un.run[1].cnt, e3 = e2 + W * un.run[2].cnt, e4 = e3 + W * un.run[3].cnt;
    const f64x2 *b0 = run_base(un.run[0]), *b1 = run_base(un.run[1]) - e1, *b2 = run_base(un.run[2]) - e2, *b3 = run_base(un.run[3]) - e3;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int f = tid + r * BSF;
      const int k = (f >= e1) + (f >= e2) + (f >= e3);
      const f64x2* src = (k == 0 ? b0 : k == 1 ? b1 : k == 2 ? b2 : b3) + f;
      const int tensor = k == 0 ? un.run[0].tensor : k == 1 ? un.run[1].tensor : k == 2 ? un.run[2].tensor : un.run[3].tensor;
      // (f_uu: its directions are controls, the upper half is all zeros and its tops word is not read)
      const bool need = f < e4 && !(tensor == K3H_FUU && f % W == 0);
      if (need) buf[u][r] = BWD_NT ? __builtin_nontemporal_load(src) : *src;
      else buf[u][r] = f64x2{0.0, 0.0};
    }
  }
  // this lane's output entry (UPJ * N <= BSF: one per lane) and what the workspace holds there (the dense terms K5 left),
  // requested now so that the read-modify-write at the end does not wait for a round trip of its own
  int dst = -1, dm = -1;
  double old_d = 0.0, old_m = 0.0;
  if (tid < UPJ * N) {
    const int u = tid / N, jj = tid - u * N;
    const K3hCol c = k3h_col(units[u], jj);
    if (c.need) {
      if (c.tensor == K3H_FUX) dst = OUX + c.j + c.slab * m;
      else {
        const int o = c.tensor == K3H_FXX ? OXX : OUU, ld = c.tensor == K3H_FXX ? n : m;
        dst = o + c.j + c.slab * ld;
        if (c.j > c.slab) dm = o + c.slab + c.j * ld;
      }
      old_d = C[dst];
      if (dm >= 0) old_m = C[dm];
    }
  }
  for (int i = tid; i < n; i += BSF) s_v[i] = Vx[i];
  __syncthreads();
#pragma unroll
  for (int u = 0; u < UPJ; ++u) {
    double* sp = (u & 1) ? s_p1 : s_p0;
    f64x2* st = (u & 1) ? s_t1 : s_t0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int f = tid + r * BSF;
      if (r < R - 1 || f < W * N) {
        const int jj = f / W, w = f - jj * W;
        if (w == 0) st[jj] = buf[u][r];
        else {
          const int ip = w - 1;
          const f64x2 vv = *reinterpret_cast<const f64x2*>(s_v + M + 2 * ip);
          sp[jj * HS::LD + ip] = vv.x * buf[u][r].x + vv.y * buf[u][r].y;
        }
      }
    }
    __syncthreads();
    if (tid < n) {
      const K3hCol c = k3h_col(units[u], tid);
      const int slab = c.slab, j = c.j;
      const bool xcol = c.tensor == K3H_FXX;
      double sacc = 0.0;
      if (c.need && c.tensor != K3H_FUU) {
        const f64x2 tw = st[tid];
        double top[2];
        top[0] = tw.x;                                                  // the slab's direction is an x direction (f_xx and f_ux)
        top[1] = 0.0;
        if (xcol && (j % M) != (slab % M)) top[1] = tw.y;               // (else: never written)
        // the upper half's partials, in bwd_contract's order: row pair (2 ip, 2 ip + 1), ip ascending; all others are zeros
        const int ra = slab % M, rb = xcol ? j % M : ra;
        const int lo = ra < rb ? ra : rb, hi = ra < rb ? rb : ra;
        const double tlo = ra <= rb ? top[0] : top[1], thi = ra <= rb ? (ra == rb ? 0.0 : top[1]) : top[0];
        if (lo == hi) {
          const int e = lo & ~1;
          const f64x2 vv = *reinterpret_cast<const f64x2*>(s_v + e);
          const double tx = (lo & 1) ? 0.0 : tlo, ty = (lo & 1) ? tlo : 0.0;
          sacc += vv.x * tx + vv.y * ty;
        } else if ((lo >> 1) == (hi >> 1)) {
          const f64x2 vv = *reinterpret_cast<const f64x2*>(s_v + lo);      // lo even, hi = lo + 1
          sacc += vv.x * tlo + vv.y * thi;
        } else {
          const f64x2 va = *reinterpret_cast<const f64x2*>(s_v + (lo & ~1));
          const f64x2 vb = *reinterpret_cast<const f64x2*>(s_v + (hi & ~1));
          sacc += va.x * ((lo & 1) ? 0.0 : tlo) + va.y * ((lo & 1) ? tlo : 0.0);
          sacc += vb.x * ((hi & 1) ? 0.0 : thi) + vb.y * ((hi & 1) ? thi : 0.0);
        }
      }
      const double* pj = sp + tid * HS::LD;
#pragma unroll
      for (int k = 0; k < HS::HP; ++k) sacc += pj[k];
      s_out[u * N + tid] = sacc;
    }
  }
  __syncthreads();
  if (dst >= 0) {
    const double v = s_out[tid];
    C[dst] = old_d + v;
    if (dm >= 0) C[dm] = old_m + v;
  }
}
