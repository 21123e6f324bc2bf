// bwd.hip -- backward (Riccati-like) sweep of augmented-Lagrangian DDP on gfx950.
//
// Replaces ddp_solver_t::backward_pass<primal_dual_affine_multipliers> (include/ddp/ddp_bwd.ipp:9-155).
// The recursion is strictly sequential in t; what is parallel is (a) the independent instances of
// the batch and (b), inside one step, the columns of Q_xx / Q_ux / Q_uu.  Each step is two launches:
//
//   bwd_assemble  grid (jobs, batch): job = a block of x-columns or u-columns.  Streams the
//                 timestep-contiguous slabs f_xx(:,:,c), f_ux(:,:,c), f_uu(:,:,c) once from HBM with
//                 16-byte coalesced loads, contracts them with V_x through LDS (tensor.hpp:179-198),
//                 and adds the dense terms f^T V_xx f (+ multiplier terms) of ddp_bwd.ipp:61-87.
//                 This is the HBM-bound kernel (0.25 flop/byte).
//   bwd_gains     grid (batch): LLT of Q_uu + reg I (lower triangle only, fail <=> pivot <= 0,
//                 ddp_bwd.ipp:104-105), k/K solves (:134-136), V_x / V_xx update (:142-146), all in LDS.
//
// A non-positive pivot marks the instance failed; the reg/mu rule of ddp_bwd.ipp:106-110 is applied
// on the device and the host relaunches the sweep for the failed instances only.
#include <stdio.h>
#include <stdlib.h>

#include "internal.h"

namespace {

struct BwdParams {
  Dims d;
  const int64_t* ne;
  const int64_t* Epre;
  const double *lfx, *lfxx, *lx, *lu, *lxx, *lux, *luu, *fx, *fu, *fxx, *fux, *fuu;
  const double *eq_val, *eq_x, *eq_u, *eq_xx, *eq_ux, *eq_uu;
  const double *x, *mult_val, *mult_jac;
  double *fb_origin, *fb_val, *fb_jac, *vx_trace, *vxx_trace;
  double *ws_V, *ws_Q, *reg, *mu;
  int32_t* status;
  int64_t* restarts;
  const BwdJob* jobs;
  const BwdJob* jobs_half;   // K3h's job list (bwd_split.h: bwd_contract_half), or null
  int32_t njobs_half;
  int32_t half_mode;         // 1: symmetric tensors with two-entry upper halves (static mode-2 stencil); 2: this context's analytic mode-1
                             // tensors -- no symmetry, the upper half of every f_xx / f_ux column and all of f_uu exact zeros
  int32_t packed;            // half_mode 1: the tensors are the stencil's packed records (lin_common.h: LinParams::pack)
  const K3hUnit* units_half; // ... read in full units (bwd_split.h: bwd_contract_units), K3H_UNITS_PER_JOB per job; or null
  int32_t njobs_units;
  const double *u, *ctrl_lo, *ctrl_hi;   // control bounds (DDP_HIP_FLAG_CONTROL_BOUNDS), else ctrl_lo / ctrl_hi null
  double* box_stat;
  int32_t has_tensors;
  int32_t sym_tensors;  // f_xx is symmetric in its two input indices bit for bit (mode-2 / zero tensors of this context's own linearisation):
                        // K3 reads one of each pair of mirrored half-slabs (bwd_split.h, job kind 2)
};

constexpr int BS = 256;
typedef double f64x2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(BS) void bwd_init(BwdParams p) {
  const int b = blockIdx.x;
  const int s = p.status[b];
  if (s == 2) return;
  const int64_t n = p.d.n;
  double* Vx = p.ws_V + (int64_t)b * (n + n * n);
  double* Vxx = Vx + n;
  const double* lfx = p.lfx + (int64_t)b * n;
  const double* lfxx = p.lfxx + (int64_t)b * n * n;
  for (int64_t i = threadIdx.x; i < n; i += BS) Vx[i] = lfx[i];        // ddp_bwd.ipp:28
  for (int64_t i = threadIdx.x; i < n * n; i += BS) Vxx[i] = lfxx[i];  // ddp_bwd.ipp:27
  __syncthreads();
  if (threadIdx.x == 0 && s == 1) p.status[b] = 0;
}

// out[j] += sum_i v[i] * Tn[i + j*O]  for j < L   (tensor_view_t::noalias_contract_add_outdim,
// detail/tensor.hpp:179-198, for one (O x L) slab = one value of the right index).
// Tn is 16-byte aligned and O is even, so a lane's 16-byte load never straddles a column.
// Stage 1: every lane loads consecutive double2's (1 KiB per wave instruction) and writes its two-term
//          partial to LDS at [column][pair] with the column stride padded to O/2+1 (bank-conflict free).
// Stage 2: lane j sums the O/2 partials of column j in a fixed order (deterministic).
template <int OC>
__device__ __forceinline__ void contract_slab(const double* __restrict__ Tn, int O_rt, int L, const double* s_v,
                                              double* s_part, double* out, int out_stride) {
  const int O = OC > 0 ? OC : O_rt;
  const int hp = O >> 1;
  const int ld = hp + 1;
  const int total = hp * L;
  const f64x2* __restrict__ T2 = reinterpret_cast<const f64x2*>(Tn);
  const int tid = threadIdx.x;
#pragma unroll 4
  for (int f = tid; f < total; f += BS) {
    const f64x2 a = __builtin_nontemporal_load(&T2[f]);
    const int j = f / hp;
    const int ip = f - j * hp;
    s_part[j * ld + ip] = s_v[2 * ip] * a.x + s_v[2 * ip + 1] * a.y;
  }
  __syncthreads();
  for (int j = tid; j < L; j += BS) {
    double s = 0.0;
    const double* pj = s_part + j * ld;
    for (int k = 0; k < hp; ++k) s += pj[k];
    out[j * out_stride] += s;
  }
  __syncthreads();
}

template <int NC, int MC>
__global__ __launch_bounds__(BS) void bwd_assemble(BwdParams p, int64_t t) {
  const int b = blockIdx.y;
  if (p.status[b] != 0) return;
  const BwdJob job = p.jobs[blockIdx.x];
  const int n = NC > 0 ? NC : (int)p.d.n;
  const int m = MC > 0 ? MC : (int)p.d.m;
  const int64_t T = p.d.T;
  const int e = (int)p.ne[t];
  const int64_t Eo = p.Epre[t];
  const int64_t Etot = p.d.Etot;
  const double mu = p.mu[b];
  const int tid = threadIdx.x;
  const int kind = job.kind, c0 = job.c0, cn = job.cn;
  const int rows = kind == 0 ? n + m : m;

  const double* Vx = p.ws_V + (int64_t)b * (n + (int64_t)n * n);
  const double* Vxx = Vx + n;
  double* Q = p.ws_Q + (int64_t)b * (n + m + (int64_t)n * n + (int64_t)m * n + (int64_t)m * m);
  double* Qx = Q;
  double* Qu = Qx + n;
  double* Qxx = Qu + m;
  double* Qux = Qxx + (int64_t)n * n;
  double* Quu = Qux + (int64_t)m * n;

  const int64_t bt = (int64_t)b * T + t;
  const double* fx = p.fx + bt * n * n;
  const double* fu = p.fu + bt * n * m;
  const double* eqv = p.eq_val + (int64_t)b * Etot + Eo;
  const double* eqx = p.eq_x + ((int64_t)b * Etot + Eo) * n;
  const double* equ = p.eq_u + ((int64_t)b * Etot + Eo) * m;
  const double* pe = p.mult_val + (int64_t)b * Etot + Eo;
  const double* pex = p.mult_jac + ((int64_t)b * Etot + Eo) * n;

  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* s_v = smem;                         // n
  double* s_tmp = s_v + n;                    // emax (>= e)
  double* s_W = s_tmp + p.d.emax;             // n * cn
  double* s_out = s_W + n * cn;               // rows * cn
  double* s_part = s_out + (n + m) * cn;      // (n/2+1) * max(n,m)

  for (int i = tid; i < n; i += BS) s_v[i] = Vx[i];
  for (int i = tid; i < e; i += BS) s_tmp[i] = pe[i] + mu * eqv[i];   // ddp_bwd.ipp:46
  __syncthreads();

  // W = V_xx * F(:, c0:c0+cn)  with F = f_x (x-job) or f_u (u-job)
  const double* Fc = (kind == 0 ? fx : fu) + (int64_t)c0 * n;
  for (int idx = tid; idx < n * cn; idx += BS) {
    const int r = idx % n, c = idx / n;
    double s = 0.0;
    for (int l = 0; l < n; ++l) s += Vxx[r + l * n] * Fc[l + c * n];
    s_W[idx] = s;
  }
  __syncthreads();

  // dense terms, in the reference's order: l, f^T V_xx f, then the multiplier terms
  for (int idx = tid; idx < rows * cn; idx += BS) {
    const int r = idx % rows, c = idx / rows;
    const int col = c0 + c;
    double acc;
    const double* Fr;
    if (kind == 0) {
      if (r < n) { acc = p.lxx[bt * n * n + r + (int64_t)col * n]; Fr = fx + (int64_t)r * n; }          // :70-71
      else { acc = p.lux[bt * m * n + (r - n) + (int64_t)col * m]; Fr = fu + (int64_t)(r - n) * n; }   // :83-84
    } else {
      acc = p.luu[bt * m * m + r + (int64_t)col * m]; Fr = fu + (int64_t)r * n;                         // :77-78
    }
    double s = 0.0;
    for (int l = 0; l < n; ++l) s += Fr[l] * s_W[l + c * n];
    acc += s;
    if (e > 0) {
      if (kind == 0) {
        if (r < n) {
          double s1 = 0.0, s2 = 0.0;
          for (int i = 0; i < e; ++i) {
            const double tmp2 = pex[i + col * e] + mu * eqx[i + col * e];   // :47
            s1 += eqx[i + r * e] * tmp2;                                     // :72
            s2 += pex[i + r * e] * eqx[i + col * e];                         // :73
          }
          acc += s1;
          acc += s2;
        } else {
          double s1 = 0.0;
          for (int i = 0; i < e; ++i) s1 += equ[i + (r - n) * e] * (pex[i + col * e] + mu * eqx[i + col * e]);  // :85
          acc += s1;
        }
      } else {
        double s1 = 0.0;
        for (int i = 0; i < e; ++i) s1 += equ[i + r * e] * equ[i + col * e];
        acc += s1 * mu;                                                      // :79
      }
      if (p.has_tensors) {
        // multiplier-weighted constraint tensors (:74, :80, :86); e is small, done in place
        const double* Te;
        int Ld;
        int jrow;
        if (kind == 0) {
          if (r < n) { Te = p.eq_xx + ((int64_t)b * Etot + Eo) * n * n; Ld = n; jrow = r; }
          else { Te = p.eq_ux + ((int64_t)b * Etot + Eo) * m * n; Ld = m; jrow = r - n; }
        } else { Te = p.eq_uu + ((int64_t)b * Etot + Eo) * m * m; Ld = m; jrow = r; }
        double s3 = 0.0;
        const double* col_ptr = Te + ((int64_t)jrow + (int64_t)col * Ld) * e;
        for (int i = 0; i < e; ++i) s3 += s_tmp[i] * col_ptr[i];
        acc += s3;
      }
    }
    s_out[idx] = acc;
  }
  // Q_x / Q_u entries of this job's columns (:61-68)
  for (int c = tid; c < cn; c += BS) {
    const int col = c0 + c;
    double acc, s = 0.0;
    if (kind == 0) {
      acc = p.lx[bt * n + col];
      for (int l = 0; l < n; ++l) s += fx[l + (int64_t)col * n] * s_v[l];
      acc += s;
      double s1 = 0.0, s2 = 0.0;
      for (int i = 0; i < e; ++i) { s1 += eqx[i + col * e] * s_tmp[i]; s2 += pex[i + col * e] * eqv[i]; }
      acc += s1;
      acc += s2;
      Qx[col] = acc;
    } else {
      acc = p.lu[bt * m + col];
      for (int l = 0; l < n; ++l) s += fu[l + (int64_t)col * n] * s_v[l];
      acc += s;
      double s1 = 0.0;
      for (int i = 0; i < e; ++i) s1 += equ[i + col * e] * s_tmp[i];
      acc += s1;
      Qu[col] = acc;
    }
  }
  __syncthreads();

  // second-order dynamics tensors contracted with V_x (:75, :81, :87): the HBM stream
  if (p.has_tensors) {
    for (int c = 0; c < cn; ++c) {
      const int col = c0 + c;
      if (kind == 0) {
        const double* Txx = p.fxx + (bt * n + col) * (int64_t)n * n;   // f_xx(:,:,col): n x n slab
        contract_slab<NC>(Txx, n, n, s_v, s_part, s_out + c * rows, 1);
        const double* Tux = p.fux + (bt * n + col) * (int64_t)n * m;   // f_ux(:,:,col): n x m slab
        contract_slab<NC>(Tux, n, m, s_v, s_part, s_out + c * rows + n, 1);
      } else {
        const double* Tuu = p.fuu + (bt * m + col) * (int64_t)n * m;   // f_uu(:,:,col): n x m slab
        contract_slab<NC>(Tuu, n, m, s_v, s_part, s_out + c * rows, 1);
      }
    }
  }

  for (int idx = tid; idx < rows * cn; idx += BS) {
    const int r = idx % rows, c = idx / rows;
    const int col = c0 + c;
    if (kind == 0) {
      if (r < n) Qxx[r + (int64_t)col * n] = s_out[idx];
      else Qux[(r - n) + (int64_t)col * m] = s_out[idx];
    } else {
      Quu[r + (int64_t)col * m] = s_out[idx];
    }
  }
}

// ---- control bounds (ddp_hip.h: DDP_HIP_FLAG_CONTROL_BOUNDS): the box QP of one step by projected Newton iterations ----
constexpr int BOX_MAX_ITER = 32;      // projected-Newton iterations per step
constexpr int BOX_MAX_HALVINGS = 33;  // step sizes 2^0 .. 2^-33 of one Armijo search
constexpr double BOX_ARMIJO = 0.1;
constexpr double BOX_GRAD_TOL = 1e-10;

__device__ __forceinline__ double box_clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// workgroup-level pieces of the box QP for bwd_gains (any shape, m <= 64 <= BS): every lane runs them, the results are uniform.
// LLT of the lower triangle of A in place, the arithmetic of bwd_gains' own loop; true <=> a pivot <= 0
__device__ bool box_llt(double* A, int lda, int m, int tid) {
  for (int k = 0; k < m; ++k) {
    const double piv = A[k + k * lda];
    if (piv <= 0.0) return true;
    const double dk = sqrt(piv);
    for (int i = k + 1 + tid; i < m; i += BS) A[i + k * lda] = A[i + k * lda] / dk;
    __syncthreads();
    const int w = m - k - 1;
    for (int idx = tid; idx < w * w; idx += BS) {
      const int i = k + 1 + idx % w, j = k + 1 + idx / w;
      if (j <= i) A[i + j * lda] -= A[i + k * lda] * A[j + k * lda];
    }
    if (tid == 0) A[k + k * lda] = dk;
    __syncthreads();
  }
  return false;
}
// r <- (L L^T)^-1 r, one right-hand side, lane = row
__device__ void box_solve(const double* A, int lda, int m, double* r, int tid) {
  for (int k = 0; k < m; ++k) {
    const double yk = r[k] / A[k + k * lda];
    __syncthreads();
    if (tid == k) r[k] = yk;
    else if (tid > k && tid < m) r[tid] -= A[tid + k * lda] * yk;
    __syncthreads();
  }
  for (int k = m - 1; k >= 0; --k) {
    const double xk = r[k] / A[k + k * lda];
    __syncthreads();
    if (tid == k) r[k] = xk;
    else if (tid < k) r[tid] -= A[k + tid * lda] * xk;
    __syncthreads();
  }
}
// obj(v) = 1/2 v^T H v + g^T v, summed in index order
__device__ double box_obj(const double* H, int lda, int m, const double* g, const double* v, double* tmp, int tid) {
  if (tid < m) {
    double s = 0.0;
    for (int j = 0; j < m; ++j) s += H[tid + j * lda] * v[j];
    tmp[tid] = v[tid] * (0.5 * s + g[tid]);
  }
  __syncthreads();
  double o = 0.0;
  for (int j = 0; j < m; ++j) o += tmp[j];
  __syncthreads();
  return o;
}

template <int NC, int MC, bool BOX = false>
__global__ __launch_bounds__(BS) void bwd_gains(BwdParams p, int64_t t) {
  const int b = blockIdx.x;
  if (p.status[b] != 0) return;
  const int n = NC > 0 ? NC : (int)p.d.n;
  const int m = MC > 0 ? MC : (int)p.d.m;
  const int nx = (int)p.d.nx;
  const int64_t T = p.d.T;
  const int tid = threadIdx.x;
  const int64_t bt = (int64_t)b * T + t;

  double* Vx = p.ws_V + (int64_t)b * (n + (int64_t)n * n);
  double* Vxx = Vx + n;
  const double* Q = p.ws_Q + (int64_t)b * (n + m + (int64_t)n * n + (int64_t)m * n + (int64_t)m * m);
  const double* Qx = Q;
  const double* Qu = Qx + n;
  const double* Qxx = Qu + m;
  const double* Qux = Qxx + (int64_t)n * n;
  const double* Quu = Qux + (int64_t)m * n;

  const int lda = m | 1;   // odd leading dimensions: column walks by the lanes are bank-conflict free
  const int ldr = m | 1;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* A = smem;                    // lda * m      Q_uu + reg I, then its Cholesky factor (lower)
  double* R = A + lda * m;             // ldr * (n+1)  [-Q_u | -Q_ux] -> [k | K]
  double* S = R + ldr * (n + 1);       // ldr * n      Q_ux

  const double reg = p.reg[b];
  bool failed = false;
  if constexpr (BOX) {
    // The box QP (ddp_hip.h).  H = the symmetric matrix of the lower triangle of Q_uu + reg I; x starts at clip(0); every
    // iteration factorises the masked matrix (rows and columns of clamped indices replaced by the identity's: LLT(H') is
    // LLT(H_ff) with ones on the clamped diagonal) and searches along the projected Newton direction
    double* H = S + ldr * n;             // lda * m
    double* g = H + lda * m;             // m each: Q_u, x, lo - u, hi - u, gradient, direction, candidate, scratch
    double *bx = g + m, *bl = bx + m, *bh = bl + m, *gr = bh + m, *dxv = gr + m, *xc = dxv + m, *tmp = xc + m;
    int* cl = reinterpret_cast<int*>(tmp + m);
    for (int idx = tid; idx < m * m; idx += BS) {
      const int i = idx % m, j = idx / m;
      H[i + j * lda] = (i >= j ? Quu[i + j * m] : Quu[j + i * m]) + (i == j ? reg : 0.0);
    }
    if (tid < m) {
      const double ut = p.u[bt * m + tid];
      const double lo = p.ctrl_lo[bt * m + tid] - ut, hi = p.ctrl_hi[bt * m + tid] - ut;
      g[tid] = Qu[tid]; bl[tid] = lo; bh[tid] = hi;
      bx[tid] = box_clip(0.0, lo, hi);
    }
    __syncthreads();
    double gabs = 0.0;
    for (int j = 0; j < m; ++j) gabs = fmax(gabs, fabs(g[j]));
    const double tol = BOX_GRAD_TOL * fmax(1.0, gabs);
    int iters = 0, nclamped = 0;
    for (;; ++iters) {
      if (tid < m) {
        double s = 0.0;
        for (int j = 0; j < m; ++j) s += H[tid + j * lda] * bx[j];
        const double gv = g[tid] + s;
        gr[tid] = gv;
        cl[tid] = ((bx[tid] <= bl[tid] && gv > 0.0) || (bx[tid] >= bh[tid] && gv < 0.0)) ? 1 : 0;
      }
      __syncthreads();
      double gmax = 0.0;
      nclamped = 0;
      for (int j = 0; j < m; ++j) { if (cl[j]) ++nclamped; else gmax = fmax(gmax, fabs(gr[j])); }
      if (nclamped == m || gmax <= tol || iters == BOX_MAX_ITER) break;
      for (int idx = tid; idx < m * m; idx += BS) {
        const int i = idx % m, j = idx / m;
        if (i >= j) A[i + j * lda] = (cl[i] || cl[j]) ? (i == j ? 1.0 : 0.0) : H[i + j * lda];
      }
      if (tid < m) dxv[tid] = cl[tid] ? 0.0 : -gr[tid];
      __syncthreads();
      failed = box_llt(A, lda, m, tid);
      if (failed) break;
      box_solve(A, lda, m, dxv, tid);
      const double o0 = box_obj(H, lda, m, g, bx, tmp, tid);
      bool taken = false;
      double a = 1.0;
      for (int hv = 0; hv <= BOX_MAX_HALVINGS && !taken; ++hv, a *= 0.5) {
        if (tid < m) xc[tid] = box_clip(bx[tid] + a * dxv[tid], bl[tid], bh[tid]);
        __syncthreads();
        double gd = 0.0;
        for (int j = 0; j < m; ++j) gd += gr[j] * (xc[j] - bx[j]);
        const double o1 = box_obj(H, lda, m, g, xc, tmp, tid);   // (ends on a barrier: the next candidate may overwrite xc)
        taken = o1 - o0 <= BOX_ARMIJO * gd;
      }
      if (!taken) break;                 // no step size accepted: x stays
      __syncthreads();
      if (tid < m) bx[tid] = xc[tid];
      __syncthreads();
    }
    if (!failed) {
      // polish on the final clamped set: with an empty set, operation for operation, the step without bounds
      for (int idx = tid; idx < m * m; idx += BS) {
        const int i = idx % m, j = idx / m;
        if (i >= j) A[i + j * lda] = (cl[i] || cl[j]) ? (i == j ? 1.0 : 0.0) : H[i + j * lda];
      }
      if (tid < m) {
        double r0;
        if (cl[tid]) r0 = bx[tid];                                           // k_c: its bound
        else if (nclamped == 0) r0 = -Qu[tid];
        else {
          double s = 0.0;
          for (int j = 0; j < m; ++j) if (cl[j]) s += H[tid + j * lda] * bx[j];
          r0 = -(g[tid] + s);                                                // -(g_f + H_fc k_c)
        }
        R[tid] = r0;
      }
      for (int idx = tid; idx < m * n; idx += BS) {
        const int i = idx % m, j = idx / m;
        const double q = Qux[idx];
        R[i + (j + 1) * ldr] = cl[i] ? 0.0 : -q;                             // K_c = 0
        S[i + j * ldr] = q;
      }
      if (tid == 0) { p.box_stat[bt * 2] = (double)nclamped; p.box_stat[bt * 2 + 1] = (double)iters; }
    }
  } else {
  for (int idx = tid; idx < m * m; idx += BS) {
    const int i = idx % m, j = idx / m;
    A[i + j * lda] = Quu[idx] + (i == j ? reg : 0.0);                        // ddp_bwd.ipp:104
  }
  for (int i = tid; i < m; i += BS) R[i] = -Qu[i];                           // :135
  for (int idx = tid; idx < m * n; idx += BS) {
    const int i = idx % m, j = idx / m;
    const double q = Qux[idx];
    R[i + (j + 1) * ldr] = -q;                                               // :136
    S[i + j * ldr] = q;
  }
  }
  __syncthreads();

  // Cholesky, lower triangle only; the update order per entry (k ascending) equals the left-looking
  // order of Eigen's unblocked LLT.  Failure <=> a pivot is <= 0.
  for (int k = 0; k < m && !failed; ++k) {
    const double piv = A[k + k * lda];
    if (piv <= 0.0) { failed = true; break; }
    const double dk = sqrt(piv);
    for (int i = k + 1 + tid; i < m; i += BS) A[i + k * lda] = A[i + k * lda] / dk;
    __syncthreads();
    const int w = m - k - 1;
    for (int idx = tid; idx < w * w; idx += BS) {
      const int i = k + 1 + idx % w, j = k + 1 + idx / w;
      if (j <= i) A[i + j * lda] -= A[i + k * lda] * A[j + k * lda];
    }
    if (tid == 0) A[k + k * lda] = dk;
    __syncthreads();
  }
  if (failed) {
    if (tid == 0) {
      double r = p.reg[b], mu = p.mu[b];
      if (r < mu) r = mu;          // ddp_bwd.ipp:106-108
      mu *= 2;                     // :109
      r *= 2;                      // :110
      p.reg[b] = r;
      p.mu[b] = mu;
      p.status[b] = 1;
      p.restarts[b] += 1;
    }
    return;
  }

  // k = -(L L^T)^-1 Q_u,  K = -(L L^T)^-1 Q_ux: one right-hand side per lane
  for (int c = tid; c < n + 1; c += BS) {
    double* r = R + c * ldr;
    for (int i = 0; i < m; ++i) {
      double s = r[i];
      for (int l = 0; l < i; ++l) s -= A[i + l * lda] * r[l];
      r[i] = s / A[i + i * lda];
    }
    for (int i = m - 1; i >= 0; --i) {
      double s = r[i];
      for (int l = i + 1; l < m; ++l) s -= A[l + i * lda] * r[l];
      r[i] = s / A[i + i * lda];
    }
  }
  __syncthreads();

  double* fbo = p.fb_origin + bt * nx;
  double* fbk = p.fb_val + bt * m;
  double* fbK = p.fb_jac + bt * m * n;
  const double* xt = p.x + ((int64_t)b * (T + 1) + t) * nx;
  for (int i = tid; i < nx; i += BS) fbo[i] = xt[i];                         // :134
  for (int i = tid; i < m; i += BS) fbk[i] = R[i];
  for (int idx = tid; idx < m * n; idx += BS) fbK[idx] = R[idx % m + (idx / m + 1) * ldr];

  // V_x = Q_x + Q_ux^T k (:142-143);  V_xx = Q_xx + Q_ux^T K (:145-146)
  for (int i = tid; i < n; i += BS) {
    double s = 0.0;
    for (int l = 0; l < m; ++l) s += S[l + i * ldr] * R[l];
    const double v = Qx[i] + s;
    Vx[i] = v;
    if (p.vx_trace) p.vx_trace[bt * n + i] = v;
  }
  for (int idx = tid; idx < n * n; idx += BS) {
    const int i = idx % n, j = idx / n;
    double s = 0.0;
    const double* si = S + i * ldr;
    const double* kj = R + (j + 1) * ldr;
    for (int l = 0; l < m; ++l) s += si[l] * kj[l];
    const double v = Qxx[idx] + s;
    Vxx[idx] = v;
    if (p.vxx_trace) p.vxx_trace[bt * n * n + idx] = v;
  }
  if (t == 0 && tid == 0) p.status[b] = 2;                                   // :149-151
}

#include "bwd_fast.h"
#include "bwd_split.h"
#include "bwd_v2.h"

size_t assemble_lds_bytes(const ddp_hip_ctx* ctx, int cn_max) {
  const Dims& d = ctx->d;
  int64_t L = d.n > d.m ? d.n : d.m;
  int64_t words = d.n + d.emax + d.n * cn_max + (d.n + d.m) * cn_max + (d.n / 2 + 1) * L;
  return (size_t)words * sizeof(double);
}
size_t gains_lds_bytes(const ddp_hip_ctx* ctx) {
  const Dims& d = ctx->d;
  int64_t ld = d.m | 1;
  int64_t words = ld * d.m + ld * (d.n + 1) + ld * d.n;
  if (ctx->flags & DDP_HIP_FLAG_CONTROL_BOUNDS) words += ld * d.m + 9 * d.m;   // H, eight vectors and the clamp flags of the box QP
  return (size_t)words * sizeof(double);
}

BwdParams make_params(ddp_hip_ctx* ctx, const SweepPlan& plan) {
  BwdParams p{};
  p.d = ctx->d;
  p.ne = ctx->ne_d;
  p.Epre = ctx->Epre_d;
  auto S = [&](int s) { return ctx->seq[s].ptr; };
  p.lfx = S(DDP_HIP_SEQ_LFX); p.lfxx = S(DDP_HIP_SEQ_LFXX);
  p.lx = S(DDP_HIP_SEQ_LX); p.lu = S(DDP_HIP_SEQ_LU); p.lxx = S(DDP_HIP_SEQ_LXX); p.lux = S(DDP_HIP_SEQ_LUX); p.luu = S(DDP_HIP_SEQ_LUU);
  p.fx = S(DDP_HIP_SEQ_FX); p.fu = S(DDP_HIP_SEQ_FU);
  p.fxx = S(DDP_HIP_SEQ_FXX); p.fux = S(DDP_HIP_SEQ_FUX); p.fuu = S(DDP_HIP_SEQ_FUU);
  p.eq_val = S(DDP_HIP_SEQ_EQ_VAL); p.eq_x = S(DDP_HIP_SEQ_EQ_X); p.eq_u = S(DDP_HIP_SEQ_EQ_U);
  p.eq_xx = S(DDP_HIP_SEQ_EQ_XX); p.eq_ux = S(DDP_HIP_SEQ_EQ_UX); p.eq_uu = S(DDP_HIP_SEQ_EQ_UU);
  p.x = S(DDP_HIP_SEQ_X);
  p.u = S(DDP_HIP_SEQ_U); p.ctrl_lo = S(DDP_HIP_SEQ_CTRL_LO); p.ctrl_hi = S(DDP_HIP_SEQ_CTRL_HI); p.box_stat = S(DDP_HIP_SEQ_BOX_STAT);
  p.mult_val = S(DDP_HIP_SEQ_MULT_VAL); p.mult_jac = S(DDP_HIP_SEQ_MULT_JAC);
  p.fb_origin = S(DDP_HIP_SEQ_FB_ORIGIN); p.fb_val = S(DDP_HIP_SEQ_FB_VAL); p.fb_jac = S(DDP_HIP_SEQ_FB_JAC);
  p.vx_trace = S(DDP_HIP_SEQ_VX_TRACE); p.vxx_trace = S(DDP_HIP_SEQ_VXX_TRACE);
  p.ws_V = ctx->ws_V; p.ws_Q = ctx->ws_Q; p.reg = ctx->reg_d; p.mu = ctx->mu_d;
  p.status = ctx->status_d; p.restarts = ctx->restarts_d;
  p.sym_tensors = plan.sym ? 1 : 0;
  p.jobs = plan.sym ? ctx->jobs_sym_d : ctx->jobs_d;
  p.jobs_half = plan.half_mode ? ctx->jobs_half_d : nullptr;
  p.njobs_half = plan.half_mode ? ctx->njobs_half : 0;
  p.half_mode = plan.half_mode;
  p.packed = plan.packed ? 1 : 0;
  const bool full_units = plan.half_mode == 1 && plan.packed && !ctx->sw.k3h_column_jobs;
  p.units_half = full_units ? ctx->units_half_d : nullptr;
  p.njobs_units = full_units ? ctx->njobs_units : 0;
  p.has_tensors = (ctx->flags & DDP_HIP_FLAG_NO_TENSORS) ? 0 : 1;
  return p;
}

template <int NC, int MC, bool BOX = false>
int launch_sweep(ddp_hip_ctx* ctx, const BwdParams& p, size_t lds_a, size_t lds_g) {
  const Dims& d = ctx->d;
  hipLaunchKernelGGL(bwd_init, dim3((unsigned)d.batch), dim3(BS), 0, ctx->stream, p);
  for (int64_t t = d.T - 1; t >= 0; --t) {
    prof_begin(ctx, DDP_HIP_K_BWD_ASSEMBLE);
    hipLaunchKernelGGL((bwd_assemble<NC, MC>), dim3((unsigned)ctx->njobs, (unsigned)d.batch), dim3(BS), lds_a, ctx->stream, p, t);
    prof_end(ctx, DDP_HIP_K_BWD_ASSEMBLE);
    prof_begin(ctx, DDP_HIP_K_BWD_GAINS);
    hipLaunchKernelGGL((bwd_gains<NC, MC, BOX>), dim3((unsigned)d.batch), dim3(BS), lds_g, ctx->stream, p, t);
    prof_end(ctx, DDP_HIP_K_BWD_GAINS);
  }
  HIP_TRY(hipGetLastError());
  return DDP_HIP_OK;
}

// three-kernel step (bwd_v2.h): K5 dense terms on 8 workgroups per instance -> K3 tensor stream (+ P) -> K4' lean Riccati
template <int NC, int MC, bool BOX>
int enqueue_sweep_v2(ddp_hip_ctx* ctx, const BwdParams& p) {
  const Dims& d = ctx->d;
  const int cn_max = ctx->cbx > ctx->cbu ? ctx->cbx : ctx->cbu;
  const size_t lds_c = sizeof(double) * (size_t)(NC + (NC + MC) * cn_max + 2 * (NC / 2 + 1) * MC);
  const size_t lds_h = sizeof(double) * (size_t)(NC + 3 * NC + 2 * (MC / 2 + 1) * NC);
  const size_t lds_u = sizeof(double) * (size_t)(NC + K3H_UNITS_PER_JOB * NC + 2 * (MC / 2 + 1) * NC + 4 * NC);
  const size_t lds_5 = sizeof(double) * (size_t)(NC * NC + NC * (NC + MC) + NC + d.emax);
  const unsigned nblk5 = (unsigned)((NC + MC + CB5 - 1) / CB5);
  const unsigned B = (unsigned)d.batch;
  hipLaunchKernelGGL(bwd_init, dim3(B), dim3(BS), 0, ctx->stream, p);
  for (int64_t t = d.T - 1; t >= 0; --t) {
    prof_begin(ctx, DDP_HIP_K_BWD_GAINS);
    hipLaunchKernelGGL((bwd_dense2<NC, MC>), dim3(nblk5, B), dim3(BS5), lds_5, ctx->stream, p, t);
    prof_end(ctx, DDP_HIP_K_BWD_GAINS);
    if (p.has_tensors) {
      prof_begin(ctx, DDP_HIP_K_BWD_ASSEMBLE);
      if (p.units_half) hipLaunchKernelGGL((bwd_contract_units<NC, MC, K3H_UNITS_PER_JOB>), dim3((unsigned)p.njobs_units, B), dim3(BSF), lds_u, ctx->stream, p, t);
      else if (p.jobs_half && p.packed) hipLaunchKernelGGL((bwd_contract_half<NC, MC, true>), dim3((unsigned)p.njobs_half, B), dim3(BSF), lds_h, ctx->stream, p, t);
      else if (p.jobs_half) hipLaunchKernelGGL((bwd_contract_half<NC, MC, false>), dim3((unsigned)p.njobs_half, B), dim3(BSF), lds_h, ctx->stream, p, t);
      else hipLaunchKernelGGL((bwd_contract<NC, MC>), dim3((unsigned)ctx->njobs, B), dim3(BSF), lds_c, ctx->stream, p, t);
      prof_end(ctx, DDP_HIP_K_BWD_ASSEMBLE);
    }
    prof_begin(ctx, DDP_HIP_K_BWD_GAINS);
    hipLaunchKernelGGL((bwd_gains2<NC, MC, BOX>), dim3(B), dim3(BS4), 0, ctx->stream, p, t);
    prof_end(ctx, DDP_HIP_K_BWD_GAINS);
  }
  HIP_TRY(hipGetLastError());
  return DDP_HIP_OK;
}

// The same enqueue, captured once into a hipGraph per state of the kernel arguments and replayed: the 600 launches of a
// sweep become one submission of a straight chain.  Profiled sweeps (HIP events around kernels) and DDP_HIP_BWD_NO_GRAPH=1
// take the direct path.
template <int NC, int MC, bool BOX>
int build_sweep_graph(ddp_hip_ctx* ctx, const BwdParams& p0, uint64_t key_misc, ddp_hip_ctx::BwdGraph** out) {
  ddp_hip_ctx::BwdGraph* slot = &ctx->bwd_graph[ctx->bwd_graph_next];
  ctx->bwd_graph_next = (ctx->bwd_graph_next + 1) % 4;
  if (slot->exec) { (void)hipGraphExecDestroy(slot->exec); slot->exec = nullptr; }
  if (slot->graph) { (void)hipGraphDestroy(slot->graph); slot->graph = nullptr; }
  HIP_TRY(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
  const int rc = enqueue_sweep_v2<NC, MC, BOX>(ctx, p0);
  hipGraph_t graph = nullptr;
  const hipError_t e = hipStreamEndCapture(ctx->stream, &graph);
  if (rc != DDP_HIP_OK || e != hipSuccess || !graph) { (void)hipGetLastError(); if (graph) (void)hipGraphDestroy(graph); return rc != DDP_HIP_OK ? rc : DDP_HIP_E_HIP; }
  hipGraphExec_t exec = nullptr;
  if (hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) { (void)hipGetLastError(); (void)hipGraphDestroy(graph); return DDP_HIP_E_HIP; }
  slot->graph = graph; slot->exec = exec; slot->key_x = p0.x; slot->key_misc = key_misc;
  *out = slot;
  return DDP_HIP_OK;
}

template <int NC, int MC, bool BOX = false>
int launch_sweep_v2(ddp_hip_ctx* ctx, const BwdParams& p0) {
  const uint32_t bwd_mask = (2u << DDP_HIP_K_BWD_ASSEMBLE) | (2u << DDP_HIP_K_BWD_GAINS);
  // profiled sweeps take the direct path: events recorded by a graph's event-record nodes cannot be read back with
  // hipEventElapsedTime on this ROCm (hipErrorInvalidHandle -- tried)
  if (ctx->sw.bwd_no_graph || (ctx->profile_mask & bwd_mask)) return enqueue_sweep_v2<NC, MC, BOX>(ctx, p0);
  const uint64_t key_misc = (uint64_t)p0.has_tensors | ((uint64_t)(p0.vx_trace != nullptr) << 1) | ((uint64_t)p0.sym_tensors << 2) | ((uint64_t)(p0.jobs_half != nullptr) << 3) | ((uint64_t)p0.half_mode << 4) | ((uint64_t)p0.packed << 8) | ((uint64_t)(p0.units_half != nullptr) << 9);
  auto find = [&](const void* key_x) -> ddp_hip_ctx::BwdGraph* {
    for (auto& g : ctx->bwd_graph)
      if (g.exec && g.key_x == key_x && g.key_misc == key_misc) return &g;
    return nullptr;
  };
  ddp_hip_ctx::BwdGraph* slot = find(p0.x);
  if (!slot) {
    int rc = build_sweep_graph<NC, MC, BOX>(ctx, p0, key_misc, &slot);
    if (rc != DDP_HIP_OK) return rc;
    // the trajectory buffers trade places after every iteration (ddp_hip_swap_traj) and x is the one kernel argument that
    // follows them: the twin graph is built now as well, so that no later sweep pays for a capture
    const double* other = ctx->seq[DDP_HIP_SEQ_X_NEW].ptr;
    if (other && other != p0.x && !find(other)) {
      BwdParams p1 = p0;
      p1.x = other;
      p1.u = ctx->seq[DDP_HIP_SEQ_U_NEW].ptr;      // (read by the box QP only: U trades places together with X)
      ddp_hip_ctx::BwdGraph* twin = nullptr;
      rc = build_sweep_graph<NC, MC, BOX>(ctx, p1, key_misc, &twin);
      if (rc != DDP_HIP_OK) return rc;
      slot = find(p0.x);
      if (!slot) return DDP_HIP_E_HIP;
    }
  }
  HIP_TRY(hipGraphLaunch(slot->exec, ctx->stream));
  return DDP_HIP_OK;
}

}  // namespace

SweepPlan sweep_plan(const ddp_hip_ctx* ctx) {
  const Dims& d = ctx->d;
  const DevSwitches& sw = ctx->sw;
  SweepPlan s{};
  // (K5 stages the multiplier jacobians over its V / F region: up to 52 constraint rows per step fit)
  s.fast = d.n == 76 && d.m == 38 && d.emax <= 52 && !sw.generic_bwd;
  s.sym_ok = s.fast && ctx->jobs_sym_d && !sw.k3_no_sym;
  const TensorOrigin o = ctx->tensors.origin;
  s.sym = s.sym_ok && (o == TensorOrigin::Symmetric || o == TensorOrigin::Stencil);
  const bool half_ok = s.fast && ctx->jobs_half_d && !sw.k3_no_half;
  // K3h needs both structural facts: symmetry and the zero configuration rows (the static stencil's own tensors) ...
  if (half_ok && s.sym && o == TensorOrigin::Stencil) { s.half_mode = 1; s.packed = ctx->tensors.packed; }   // (on the stencil's records where it left them packed)
  // ... or the structure the analytic mode-1 pass leaves (lin_analytic.hip): q+ = q + dt v has constant jacobian rows and M^-1 does
  // not depend on u, so the upper halves and f_uu are zeros it wrote itself
  else if (half_ok && o == TensorOrigin::Analytic1) s.half_mode = 2;
  return s;
}

int bwd_setup(ddp_hip_ctx* ctx) {
  const Dims& d = ctx->d;
  const int64_t n = d.n, m = d.m, B = d.batch;
  HIP_TRY(hipMalloc(&ctx->ws_V, sizeof(double) * (size_t)(B * (n + n * n))));
  HIP_TRY(hipMalloc(&ctx->ws_Q, sizeof(double) * (size_t)(B * (n + m + n * n + m * n + m * m))));
  HIP_TRY(hipMalloc(&ctx->reg_d, sizeof(double) * (size_t)B));
  HIP_TRY(hipMalloc(&ctx->mu_d, sizeof(double) * (size_t)B));
  HIP_TRY(hipMalloc(&ctx->status_d, sizeof(int32_t) * (size_t)B));
  HIP_TRY(hipMalloc(&ctx->restarts_d, sizeof(int64_t) * (size_t)B));

  // column jobs: one x-column streams 3 units (n*n + n*m doubles), one u-column 1 unit (n*m doubles);
  // aim at >= ~2048 workgroups per launch so that all 256 CUs hold several streaming workgroups
  int64_t units = 3 * n + m;
  int64_t want = 2048 / B;
  if (want < 1) want = 1;
  if (want > n + m) want = n + m;
  int64_t upj = (units + want - 1) / want;
  int64_t cbx = upj / 3; if (cbx < 1) cbx = 1; if (cbx > 8) cbx = 8;
  int64_t cbu = upj;     if (cbu < 1) cbu = 1; if (cbu > 16) cbu = 16;
  // Talos shape (K3): one x-column per job (3 units: two half-slabs of f_xx and one slab of f_ux) and three u-columns per job
  // (3 units of f_uu): 89 equal jobs of 69 KB per instance.  Measured at 64 instances: 66 us per launch (6.1 TB/s) against 74 us
  // (5.5 TB/s) for the 31 jobs of 3 / 9 columns the rule above picks.
  if (n == 76 && m == 38) { cbx = 1; cbu = 3; }
  if (ctx->sw.bwd_cbx) cbx = ctx->sw.bwd_cbx;    // tuning knobs
  if (ctx->sw.bwd_cbu) cbu = ctx->sw.bwd_cbu;
  ctx->cbx = (int32_t)cbx; ctx->cbu = (int32_t)cbu;
  std::vector<BwdJob> jobs;
  for (int64_t c = 0; c < n; c += cbx) jobs.push_back(BwdJob{0, (int32_t)c, (int32_t)((n - c) < cbx ? (n - c) : cbx), 0});
  for (int64_t c = 0; c < m; c += cbu) jobs.push_back(BwdJob{1, (int32_t)c, (int32_t)((m - c) < cbu ? (m - c) : cbu), 0});
  ctx->njobs = (int32_t)jobs.size();
  if (n == 76 && m == 38) {
    // K5 needs more than the default 64 KB of dynamic LDS.  The attribute is per device: it is set here, with the
    // context's device current, by every context (not behind a process-wide flag)
    const size_t lds_5 = sizeof(double) * (size_t)(76 * 76 + 76 * (76 + 38) + 76 + d.emax);
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&bwd_dense2<76, 38>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_5));
  }
  if ((ctx->flags & DDP_HIP_FLAG_CONTROL_BOUNDS) && gains_lds_bytes(ctx) <= 160 * 1024) {
    // the box QP keeps a second copy of Q_uu in LDS: past the default 64 KB of dynamic LDS from m = 35 on
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&bwd_gains<0, 0, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)gains_lds_bytes(ctx)));
  }
  // ... and so do the run-time-shaped kernels of every other robot: bwd_gains from nv = 40, bwd_assemble from nv = 60 (at this
  // context's job width).  A size past 160 KB gets no attribute: ddp_hip_backward refuses it (bwd_lds_check)
  {
    const size_t lds_a = assemble_lds_bytes(ctx, (int)(cbx > cbu ? cbx : cbu)), lds_g = gains_lds_bytes(ctx);
    if (lds_a > 64 * 1024 && lds_a <= 160 * 1024)
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&bwd_assemble<0, 0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_a));
    if (!(ctx->flags & DDP_HIP_FLAG_CONTROL_BOUNDS) && lds_g > 64 * 1024 && lds_g <= 160 * 1024)
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&bwd_gains<0, 0, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_g));
  }
  HIP_TRY(hipMalloc(&ctx->jobs_d, sizeof(BwdJob) * jobs.size()));
  HIP_TRY(hipMemcpy(ctx->jobs_d, jobs.data(), sizeof(BwdJob) * jobs.size(), hipMemcpyHostToDevice));
  if (n == 76 && m == 38 && cbx == 1) {
    // the same list for symmetric tensors: the x-columns c >= m skip their first half-slab (job kind 2, bwd_split.h)
    std::vector<BwdJob> js = jobs;
    for (auto& j : js) if (j.kind == 0 && j.c0 >= m) j.kind = 2;
    HIP_TRY(hipMalloc(&ctx->jobs_sym_d, sizeof(BwdJob) * js.size()));
    HIP_TRY(hipMemcpy(ctx->jobs_sym_d, js.data(), sizeof(BwdJob) * js.size(), hipMemcpyHostToDevice));
    // K3h (bwd_contract_half): x-columns in pairs (3 units each), u-columns in groups of 6 (3 units), the rest in one
    const std::vector<BwdJob> jh = k3h_column_jobs((int)n, (int)m);
    ctx->njobs_half = (int32_t)jh.size();
    HIP_TRY(hipMalloc(&ctx->jobs_half_d, sizeof(BwdJob) * jh.size()));
    HIP_TRY(hipMemcpy(ctx->jobs_half_d, jh.data(), sizeof(BwdJob) * jh.size(), hipMemcpyHostToDevice));
    // ... and the packed K3h (bwd_contract_units): the same columns in full units (bwd_jobs.h)
    std::vector<K3hUnit> us = k3h_full_units((int)n, (int)m);
    if (!k3h_units_in_bounds(us, (int)n, (int)m)) return DDP_HIP_E_ARG;
    ctx->njobs_units = k3h_pad_to_jobs(us, K3H_UNITS_PER_JOB);
    HIP_TRY(hipMalloc(&ctx->units_half_d, sizeof(K3hUnit) * us.size()));
    HIP_TRY(hipMemcpy(ctx->units_half_d, us.data(), sizeof(K3hUnit) * us.size(), hipMemcpyHostToDevice));
  }
  return DDP_HIP_OK;
}

void bwd_teardown(ddp_hip_ctx* ctx) {
  for (auto& g : ctx->bwd_graph) {
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
    if (g.graph) (void)hipGraphDestroy(g.graph);
  }
  if (ctx->ws_V) (void)hipFree(ctx->ws_V);
  if (ctx->ws_Q) (void)hipFree(ctx->ws_Q);
  if (ctx->reg_d) (void)hipFree(ctx->reg_d);
  if (ctx->mu_d) (void)hipFree(ctx->mu_d);
  if (ctx->status_d) (void)hipFree(ctx->status_d);
  if (ctx->restarts_d) (void)hipFree(ctx->restarts_d);
  if (ctx->jobs_d) (void)hipFree(ctx->jobs_d);
  if (ctx->jobs_sym_d) (void)hipFree(ctx->jobs_sym_d);
  if (ctx->jobs_half_d) (void)hipFree(ctx->jobs_half_d);
  if (ctx->units_half_d) (void)hipFree(ctx->units_half_d);
}

// The sweep's LDS against the 160 KB of a gfx950 workgroup, on the host: bwd_gains holds Q_uu, [k | K] and Q_ux, which fits up to
// nv = 63 (57 with control bounds: the box QP's second copy of Q_uu).  The Talos shape's own kernels are sized at compile time
int bwd_lds_check(const ddp_hip_ctx* ctx) {
  if (sweep_plan(ctx).fast) return DDP_HIP_OK;
  const int cn_max = ctx->cbx > ctx->cbu ? ctx->cbx : ctx->cbu;
  if (assemble_lds_bytes(ctx, cn_max) > 160 * 1024 || gains_lds_bytes(ctx) > 160 * 1024) return DDP_HIP_E_UNSUPPORTED;
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_backward(ddp_hip_ctx* ctx, double* reg_io, double* mu_io, int64_t* restarts_out, int64_t max_restarts) {
  if (!ctx || !reg_io || !mu_io) return DDP_HIP_E_ARG;
  { const int rc_ = bwd_lds_check(ctx); if (rc_ != DDP_HIP_OK) return rc_; }   // (ahead of the first launch, copy or conversion of the tensors)
  const Dims& d = ctx->d;
  const int64_t B = d.batch;
  HIP_TRY(hipSetDevice(ctx->device));
  SweepPlan plan = sweep_plan(ctx);
  // packed records are for the packed K3h alone: any other sweep reads the contract layout
  if (ctx->tensors.packed && !plan.packed) {
    const int rc_ = lin_materialize_fxx(ctx);
    if (rc_ != DDP_HIP_OK) return rc_;
    plan = sweep_plan(ctx);
  }
  BwdParams p = make_params(ctx, plan);
  if (p.has_tensors && (!p.fxx || !p.fux || !p.fuu)) return DDP_HIP_E_UNSUPPORTED;
  const bool box = (ctx->flags & DDP_HIP_FLAG_CONTROL_BOUNDS) != 0;
  if (box) { const int rc_ = box_check(ctx); if (rc_ != DDP_HIP_OK) return rc_; }
  // the static stencil leaves the f_xx block out that the symmetric sweep never reads: any other sweep needs it (the tensors
  // may have changed since the linearisation: upload / device_ptr)
  if (p.has_tensors && ctx->tensors.mirror_pending && !plan.sym) { const int rc_ = lin_materialize_fxx(ctx); if (rc_ != DDP_HIP_OK) return rc_; }

  HIP_TRY(hipMemcpyAsync(ctx->reg_d, reg_io, sizeof(double) * (size_t)B, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(ctx->mu_d, mu_io, sizeof(double) * (size_t)B, hipMemcpyHostToDevice, ctx->stream));
  std::vector<int32_t> status((size_t)B);
  for (int64_t b = 0; b < B; ++b) status[(size_t)b] = ctx->active_h[(size_t)b] ? 0 : 2;   // a frozen instance counts as done
  HIP_TRY(hipMemcpyAsync(ctx->status_d, status.data(), sizeof(int32_t) * (size_t)B, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemsetAsync(ctx->restarts_d, 0, sizeof(int64_t) * (size_t)B, ctx->stream));

  const int cn_max = ctx->cbx > ctx->cbu ? ctx->cbx : ctx->cbu;
  const size_t lds_a = assemble_lds_bytes(ctx, cn_max);
  const size_t lds_g = gains_lds_bytes(ctx);

  bool any_restart = false;
  int rc = DDP_HIP_OK;
  for (int64_t attempt = 0;; ++attempt) {
    // the Talos-like shape runs K5 / K3 / K4' (sweep_plan); every other shape the run-time-shaped pair
    // (with control bounds: the box instantiations of the gains kernels)
    if (plan.fast) rc = box ? launch_sweep_v2<76, 38, true>(ctx, p) : launch_sweep_v2<76, 38>(ctx, p);
    else if (d.n == 12 && d.m == 6) rc = box ? launch_sweep<12, 6, true>(ctx, p, lds_a, lds_g) : launch_sweep<12, 6>(ctx, p, lds_a, lds_g);
    else rc = box ? launch_sweep<0, 0, true>(ctx, p, lds_a, lds_g) : launch_sweep<0, 0>(ctx, p, lds_a, lds_g);
    if (rc != DDP_HIP_OK) return rc;
    HIP_TRY(hipMemcpyAsync(status.data(), ctx->status_d, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    bool failed = false;
    for (int64_t b = 0; b < B; ++b) failed |= status[(size_t)b] == 1;
    if (!failed) break;
    any_restart = true;
    if (max_restarts >= 0 && attempt >= max_restarts) { rc = DDP_HIP_E_MAX_RESTARTS; break; }
  }
  HIP_TRY(hipMemcpyAsync(reg_io, ctx->reg_d, sizeof(double) * (size_t)B, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipMemcpyAsync(mu_io, ctx->mu_d, sizeof(double) * (size_t)B, hipMemcpyDeviceToHost, ctx->stream));
  if (restarts_out)
    HIP_TRY(hipMemcpyAsync(restarts_out, ctx->restarts_d, sizeof(int64_t) * (size_t)B, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (rc != DDP_HIP_OK) return rc;
  return any_restart ? DDP_HIP_EV_LLT_RESTART : DDP_HIP_OK;
}

#ifdef BWD_STAMPS
extern "C" int ddp_hip_debug_stamps(unsigned long long* out32) {
  return hipMemcpyFromSymbol(out32, HIP_SYMBOL(g_bwd_stamps), sizeof(unsigned long long) * 32) == hipSuccess ? 0 : -2;
}
#endif
