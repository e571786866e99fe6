// mjb_lqr.hpp — the backward pass of a batched time-varying LQR / iLQR (mjb_lqr_backward), its control-limited form
// (mjb_lqr_backward_box) and the line search's candidate controls (mjb_lqr_candidates) as workgroup-cooperative float64 device code.
//
// One workgroup advances one trajectory: T steps in series, Vxx and every per-step temporary resident in LDS, the products on
// v_mfma_f64_16x16x4_f64 tiles (lqr_gemm_tn), the next step's (A, B) blocks in flight in registers while the current step computes.
// Consumes what mjb_transition_fd_points writes (the reference designs its controllers from one (A, B) with
// scipy.linalg.solve_discrete_are, reference examples/humanoid/controllers/lqr.py:114; this is that recursion along a trajectory).
//
// The same source compiles in a host emulation (MJB_HOST_EMU: one std::thread per lane, pthread barriers, the f64 MFMA emulated in
// its hardware fragment layout) that only the CPU test-suite uses; the product library never contains that build.
#pragma once
#include <cmath>
#include <cstddef>

#ifdef MJB_HOST_EMU
#include <pthread.h>
#define MJB_LQR_HD static inline
#define MJB_LQR_DEV static inline
#else
#include <hip/hip_runtime.h>
#define MJB_LQR_HD __host__ __device__ static inline
#define MJB_LQR_DEV __device__ __forceinline__
#endif

namespace mjb {

static const int kLqrMaxNx = 64, kLqrMaxNu = 32, kLqrMaxAlpha = 64;

// One float64 array addressed by (step, environment): element i of block (t, e) is p[t * ss + e * es + i]; strides in elements, 0 = broadcast
struct LqrStrided { const double* p; long ss, es; };

struct LqrBackwardArgs {
  int T, B, nx, nu;
  LqrStrided A, Bm, lx, lu, lxx, luu, lux;          // lux.p may be null (= 0)
  LqrStrided VxT, VxxT, mu;                         // terminal values / regularisation: env stride only
  double *k, *K, *dV, *V0x, *V0xx;                  // k [T, B, nu], K [T, B, nu, nx], dV [B, 2]; V0x [B, nx], V0xx [B, nx, nx] may be null
  int* status;                                      // [B]
};

// mjb_lqr_backward_box: the arguments above plus the nominal controls u [nu] per (t, e), the box lo / hi [nu] (null = unbounded on
// that side) and two more outputs, clamped [T, B] (bit a = control a clamped at that step) and qp_iters [B]
struct LqrBoxArgs {
  LqrBackwardArgs b;
  LqrStrided u;
  const double *lo, *hi;
  int *clamped, *qp_iters;
};

struct LqrCandArgs {
  int T, B, nx, nu, nalpha, out_f32;
  LqrStrided A, Bm, k, K, u, dx0;                   // dx0.p may be null (= 0), env stride only
  const double *alphas, *lo, *hi;                   // lo / hi [nu] may be null (unbounded)
  void* cand;                                       // [B, nalpha, T, nu] float64 or float32
};

// ---- LDS layouts (offsets in doubles) ---------------------------------------------------------------------------------------
// Backward pass.  Persistent: Vxx (holds Qxx between the products and the update), Vx, Qux, Quu, Qx, Qu, wq = Quu k.  The rest is a
// union of the two halves of a step: the products read A, B, VA = Vxx A, VB = Vxx B; the solve and the update use Qw (the working
// copy the Cholesky eliminates), L (its factor, row stride kLqrMaxNu so that the unrolled substitutions address it with constants), R = [Qux | Qu] solved in place into -[K | k], and S = Quu K + Qux.
struct LqrLay { int Vxx, Vx, Qux, Quu, Qx, Qu, wq, A, B, VA, VB, Qw, L, R, S, total; };
MJB_LQR_HD LqrLay lqr_layout(int nx, int nu) {
  LqrLay l;
  int o = 0;
  l.Vxx = o; o += nx * nx;
  l.Qux = o; o += nu * nx;
  l.Quu = o; o += nu * nu;
  l.Vx = o; o += nx;
  l.Qx = o; o += nx;
  l.Qu = o; o += nu;
  l.wq = o; o += nu;
  o = (o + 1) & ~1;
  const int u0 = o;
  l.A = o; o += nx * nx;
  l.VA = o; o += nx * nx;
  l.B = o; o += nx * nu;
  l.VB = o; o += nx * nu;
  const int end1 = o;
  o = u0;
  l.Qw = o; o += nu * nu;
  l.L = o; o += nu * kLqrMaxNu;
  l.R = o; o += nu * (nx + 1);
  l.S = o; o += nu * nx;
  l.total = o > end1 ? o : end1;
  return l;
}
// Control-limited backward pass: the layout above, and after S in the solve half of the union the QP's vectors - the iterate x, the
// Newton target xs, the gradient g, the box lob / hib of the step, the clamped and the inside-the-box flags (one word per control), and
// one flag per search trial.
static const int kLqrQpIters = 64, kLqrQpTrials = 64;            // the caps: the kernel ends in bounded time on any input
struct LqrBoxLay { LqrLay l; int x, xs, g, lob, hib, cf, fe, pass, total; };
MJB_LQR_HD LqrBoxLay lqr_box_layout(int nx, int nu) {
  LqrBoxLay b;
  b.l = lqr_layout(nx, nu);
  int o = b.l.S + nu * nx;
  b.x = o; o += nu;
  b.xs = o; o += nu;
  b.g = o; o += nu;
  b.lob = o; o += nu;
  b.hib = o; o += nu;
  b.cf = o; o += nu;
  b.fe = o; o += nu;
  b.pass = o; o += kLqrQpTrials;
  b.total = o > b.l.total ? o : b.l.total;
  return b;
}
// Candidates: the step's A (row stride nx | 1: the mat-vec reads a column of lanes down the rows), B, K (row stride nx | 1), k, u and
// per step size the deviation dx (two copies: read one, write the other) and du = c - u.
struct LqrCandLay { int A, B, K, k, u, dx, du, lda, total; };
MJB_LQR_HD LqrCandLay lqr_cand_layout(int nx, int nu, int nalpha) {
  LqrCandLay l;
  l.lda = nx | 1;
  int o = 0;
  l.A = o; o += nx * l.lda;
  l.K = o; o += nu * l.lda;
  l.B = o; o += nx * nu;
  l.k = o; o += nu;
  l.u = o; o += nu;
  l.dx = o; o += 2 * nalpha * nx;
  l.du = o; o += nalpha * nu;
  l.total = o;
  return l;
}
// Waves per workgroup of the backward kernel: one for small states (a wave-level barrier is all a step then needs), four otherwise.
// At most four 16 x 16 tiles per wave in every product either way (lqr_gemm_tn).
MJB_LQR_HD int lqr_waves(int nx) { return nx <= 16 ? 1 : 4; }

// Host arithmetic of the argument checks (no HIP: tested without a GPU).  Highest element a strided [T, B, n] array touches;
// false: an empty extent or a negative stride.  128-bit so that no stride overflows.
inline bool lqr_highest_element(long T, long B, long n, long ss, long es, __int128& hi) {
  hi = -1;
  if (T < 1 || B < 1 || n < 1 || ss < 0 || es < 0) return false;
  hi = (__int128)(T - 1) * ss + (__int128)(B - 1) * es + (n - 1);
  return true;
}
// 0 ok; otherwise which limit the sizes break (the entry points turn it into the message)
inline int lqr_size_error(long T, long B, long nx, long nu) {
  if (T < 1) return 1;
  if (B < 1) return 2;
  if (nx < 1 || nx > kLqrMaxNx) return 3;
  if (nu < 1 || nu > kLqrMaxNu) return 4;
  if ((__int128)T * B * nu * nx > ((__int128)1 << 40)) return 5;
  return 0;
}

// ---- workgroup primitives ---------------------------------------------------------------------------------------------------
#ifdef MJB_HOST_EMU
struct lqr_d4 { double v[4]; double& operator[](int i) { return v[i]; } const double& operator[](int i) const { return v[i]; } };
namespace lqremu {
struct Block {
  int nthreads;
  pthread_barrier_t bar, wbar[4];
  double a[4][2][64], b[4][2][64];
  int phase[256];
  explicit Block(int n) : nthreads(n) {
    pthread_barrier_init(&bar, nullptr, (unsigned)n);
    for (int w = 0; w < 4; w++) pthread_barrier_init(&wbar[w], nullptr, 64u);
    for (int i = 0; i < 256; i++) phase[i] = 0;
  }
  ~Block() { pthread_barrier_destroy(&bar); for (int w = 0; w < 4; w++) pthread_barrier_destroy(&wbar[w]); }
};
inline thread_local Block* tl_block = nullptr;
inline thread_local int tl_tid = 0;
}  // namespace lqremu
static inline void lqr_sync() { pthread_barrier_wait(&lqremu::tl_block->bar); }
// D = A (16 x 4) B (4 x 16) + C in the fragment layout of v_mfma_f64_16x16x4_f64: lane l gives A[l & 15][l >> 4] and B[l >> 4][l & 15]
// and holds D[(l >> 4) + 4 r][l & 15] in register r.  A collective of the 64 lane threads of one wave; the operands go through
// double-buffered scratch so that one barrier per call suffices.
static inline lqr_d4 lqr_emu_mfma(double a, double b, lqr_d4 acc) {
  lqremu::Block* g = lqremu::tl_block;
  const int tid = lqremu::tl_tid, w = tid >> 6, lane = tid & 63, p = g->phase[tid]++ & 1;
  g->a[w][p][lane] = a; g->b[w][p][lane] = b;
  pthread_barrier_wait(&g->wbar[w]);
  const int col = lane & 15;
  for (int r = 0; r < 4; r++) {
    const int row = (lane >> 4) + 4 * r;
    for (int k = 0; k < 4; k++) acc.v[r] = std::fma(g->a[w][p][row + 16 * k], g->b[w][p][col + 16 * k], acc.v[r]);
  }
  return acc;
}
#define MJB_MFMA_F64(a, b, acc) lqr_emu_mfma((a), (b), (acc))
#else
typedef double lqr_d4 __attribute__((ext_vector_type(4)));
MJB_LQR_DEV void lqr_sync() { __syncthreads(); }
#define MJB_MFMA_F64(a, b, acc) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (acc), 0, 0, 0)
#endif

// C [M, N] = init + sum_k a[k * lda + i] * b[k * ldb + j]  (+ sum_k a2[k * lda2 + i] * b2[k * ldb2 + j] over K2, 0 = none): both
// operands are read along their rows (k outer), i.e. the left factor is given TRANSPOSED - every product of the recursion has that
// form (Vxx and Quu are symmetric), so no LDS read walks a column.  The 16 x 16 output tiles go round the NW waves, at most four per
// wave (M, N <= 64 with four waves, M * N <= 1024 with one), each with its own accumulator so that consecutive MFMAs are independent.
// Rows / columns / k beyond the extents are fed as zeros.  init(row, col) and store(row, col, value) run once per element.
template <int NW, class Init, class Store>
MJB_LQR_DEV void lqr_gemm_tn(int M, int N, int K, const double* a, int lda, const double* b, int ldb,
                             int K2, const double* a2, int lda2, const double* b2, int ldb2, int tid, Init init, Store store) {
  const int wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
  const int nt = (N + 15) >> 4, ntile = ((M + 15) >> 4) * nt;
  lqr_d4 acc[4];
  int ti[4], tj[4];
  bool on[4];
#pragma unroll
  for (int s = 0; s < 4; s++) {
    const int q = wave + NW * s;
    on[s] = q < ntile;
    ti[s] = 16 * (q / nt); tj[s] = 16 * (q % nt);
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = ti[s] + lk + 4 * r, col = tj[s] + li;
      acc[s][r] = (on[s] && row < M && col < N) ? init(row, col) : 0.0;
    }
  }
  for (int k0 = 0; k0 < K; k0 += 4) {
    const int k = k0 + lk;
#pragma unroll
    for (int s = 0; s < 4; s++) {
      if (!on[s]) continue;                                      // wave-uniform
      const int i = ti[s] + li, j = tj[s] + li;
      const double av = (k < K && i < M) ? a[k * lda + i] : 0.0, bv = (k < K && j < N) ? b[k * ldb + j] : 0.0;
      acc[s] = MJB_MFMA_F64(av, bv, acc[s]);
    }
  }
  for (int k0 = 0; k0 < K2; k0 += 4) {
    const int k = k0 + lk;
#pragma unroll
    for (int s = 0; s < 4; s++) {
      if (!on[s]) continue;
      const int i = ti[s] + li, j = tj[s] + li;
      const double av = (k < K2 && i < M) ? a2[k * lda2 + i] : 0.0, bv = (k < K2 && j < N) ? b2[k * ldb2 + j] : 0.0;
      acc[s] = MJB_MFMA_F64(av, bv, acc[s]);
    }
  }
#pragma unroll
  for (int s = 0; s < 4; s++) {
    if (!on[s]) continue;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = ti[s] + lk + 4 * r, col = tj[s] + li;
      if (row < M && col < N) store(row, col, acc[s][r]);
    }
  }
}

// C [M, N] = a^T b for a [K, M], b [K, N] in global memory: the helper on its own (the fragment-layout test)
template <int NW>
MJB_LQR_DEV void lqr_gemm_probe(int M, int N, int K, const double* a, const double* b, double* c, int tid) {
  lqr_gemm_tn<NW>(M, N, K, a, M, b, N, 0, nullptr, 0, nullptr, 0, tid, [](int, int) { return 0.0; },
                  [&](int row, int col, double v) { c[row * N + col] = v; });
}

// ---- the pieces of one step, shared by lqr_backward_env and lqr_backward_box_env ----------------------------------------------
struct LqrLds { double *Vxx, *Vx, *Qux, *Quu, *Qx, *Qu, *wq, *A, *B, *VA, *VB, *Qw, *L, *R, *S; };
MJB_LQR_DEV LqrLds lqr_lds_pointers(double* w, const LqrLay& l) {
  LqrLds m;
  m.Vxx = w + l.Vxx; m.Vx = w + l.Vx; m.Qux = w + l.Qux; m.Quu = w + l.Quu; m.Qx = w + l.Qx; m.Qu = w + l.Qu; m.wq = w + l.wq;
  m.A = w + l.A; m.B = w + l.B; m.VA = w + l.VA; m.VB = w + l.VB; m.Qw = w + l.Qw; m.L = w + l.L; m.R = w + l.R; m.S = w + l.S;
  return m;
}

// Vxx = VxxT, Vx = VxT and the last step's (A, B) into LDS
template <int NT>
MJB_LQR_DEV void lqr_load_terminal(const LqrBackwardArgs& p, int e, const LqrLds& m, int tid) {
  const int nx = p.nx, nu = p.nu;
  const double* Ag = p.A.p + (long)e * p.A.es;
  const double* Bg = p.Bm.p + (long)e * p.Bm.es;
  for (int i = tid; i < nx * nx; i += NT) m.Vxx[i] = p.VxxT.p[(long)e * p.VxxT.es + i];
  for (int i = tid; i < nx; i += NT) m.Vx[i] = p.VxT.p[(long)e * p.VxT.es + i];
  for (int i = tid; i < nx * nx; i += NT) m.A[i] = Ag[(long)(p.T - 1) * p.A.ss + i];
  for (int i = tid; i < nx * nu; i += NT) m.B[i] = Bg[(long)(p.T - 1) * p.Bm.ss + i];
  lqr_sync();
}

// the blocks of step t - 1 into registers (zeros at t = 0): issued at the start of step t, written to LDS at its end (lqr_step_end)
template <int NT, int PA, int PB>
MJB_LQR_DEV void lqr_prefetch(const LqrBackwardArgs& p, int t, int e, int tid, double (&ra)[PA], double (&rb)[PB]) {
  const int nx = p.nx, nu = p.nu;
  const double* Ag = p.A.p + (long)e * p.A.es;
  const double* Bg = p.Bm.p + (long)e * p.Bm.es;
#pragma unroll
  for (int n = 0; n < PA; n++) { const int i = tid + n * NT; ra[n] = (t > 0 && i < nx * nx) ? Ag[(long)(t - 1) * p.A.ss + i] : 0.0; }
#pragma unroll
  for (int n = 0; n < PB; n++) { const int i = tid + n * NT; rb[n] = (t > 0 && i < nx * nu) ? Bg[(long)(t - 1) * p.Bm.ss + i] : 0.0; }
}

// VA = Vxx A, VB = Vxx B, then Qxx = lxx + A^T VA (into Vxx, which nothing reads any more), Qux = lux + B^T VA,
// Quu = luu + B^T VB + mu I, Qx = lx + A^T Vx, Qu = lu + B^T Vx
template <int NW>
MJB_LQR_DEV void lqr_step_products(const LqrBackwardArgs& p, int t, int e, double mu, const LqrLds& m, int tid) {
  constexpr int NT = 64 * NW;
  const int nx = p.nx, nu = p.nu;
  double *Vxx = m.Vxx, *Vx = m.Vx, *Qux = m.Qux, *Quu = m.Quu, *Qx = m.Qx, *Qu = m.Qu, *A = m.A, *Bt = m.B, *VA = m.VA, *VB = m.VB;
  lqr_gemm_tn<NW>(nx, nx, nx, Vxx, nx, A, nx, 0, nullptr, 0, nullptr, 0, tid, [](int, int) { return 0.0; },
                  [&](int r, int c, double v) { VA[r * nx + c] = v; });
  lqr_gemm_tn<NW>(nx, nu, nx, Vxx, nx, Bt, nu, 0, nullptr, 0, nullptr, 0, tid, [](int, int) { return 0.0; },
                  [&](int r, int c, double v) { VB[r * nu + c] = v; });
  lqr_sync();

  const double* lxx = p.lxx.p + (long)t * p.lxx.ss + (long)e * p.lxx.es;
  const double* luu = p.luu.p + (long)t * p.luu.ss + (long)e * p.luu.es;
  const double* lux = p.lux.p ? p.lux.p + (long)t * p.lux.ss + (long)e * p.lux.es : nullptr;
  lqr_gemm_tn<NW>(nx, nx, nx, A, nx, VA, nx, 0, nullptr, 0, nullptr, 0, tid, [&](int r, int c) { return lxx[r * nx + c]; },
                  [&](int r, int c, double v) { Vxx[r * nx + c] = v; });
  lqr_gemm_tn<NW>(nu, nx, nx, Bt, nu, VA, nx, 0, nullptr, 0, nullptr, 0, tid, [&](int r, int c) { return lux ? lux[r * nx + c] : 0.0; },
                  [&](int r, int c, double v) { Qux[r * nx + c] = v; });
  lqr_gemm_tn<NW>(nu, nu, nx, Bt, nu, VB, nu, 0, nullptr, 0, nullptr, 0, tid, [&](int r, int c) { return luu[r * nu + c] + (r == c ? mu : 0.0); },
                  [&](int r, int c, double v) { Quu[r * nu + c] = v; });
  const double* lx = p.lx.p + (long)t * p.lx.ss + (long)e * p.lx.es;
  const double* lu = p.lu.p + (long)t * p.lu.ss + (long)e * p.lu.es;
  for (int i = tid; i < nx + nu; i += NT) {
    if (i < nx) {
      double s = lx[i];
      for (int k = 0; k < nx; k++) s = fma(A[k * nx + i], Vx[k], s);
      Qx[i] = s;
    } else {
      const int a = i - nx;
      double s = lu[a];
      for (int k = 0; k < nx; k++) s = fma(Bt[k * nu + a], Vx[k], s);
      Qu[a] = s;
    }
  }
  lqr_sync();
}

// Cholesky Qw = L L^T, right-looking, one barrier per column: column j of the factor goes to L while every thread forms the
// entries of it that its own trailing updates need from Qw's column j (same operations, same values).  false at a pivot that is
// <= 0 or not finite - uniform: every thread reads the same pivot.
template <int NT>
MJB_LQR_DEV bool lqr_cholesky(double* Qw, double* Lf, int nu, int tid) {
  constexpr int ldl = kLqrMaxNu;
  for (int j = 0; j < nu; j++) {
    const double d = Qw[j * nu + j];
    if (!(d > 0.0) || !(d <= 1.7976931348623157e308)) return false;
    const double s = sqrt(d);
    for (int i = tid; i < nu * nu; i += NT) {
      const int r = i / nu, c = i % nu;
      if (r < j || c < j || c > r) continue;
      if (c == j) Lf[r * ldl + j] = r == j ? s : Qw[r * nu + j] / s;
      else Qw[r * nu + c] -= (Qw[r * nu + j] / s) * (Qw[c * nu + j] / s);
    }
    lqr_sync();
  }
  return true;
}

// L L^T x = column c of R, the column in registers: forward, backward, then store(i, -x[i]) for every row
template <int MU, class Store>
MJB_LQR_DEV void lqr_solve_column(const double* R, int ldr, const double* Lf, int nu, int c, Store store) {
  constexpr int ldl = kLqrMaxNu;
  double x[MU];
#pragma unroll
  for (int i = 0; i < MU; i++) x[i] = i < nu ? R[i * ldr + c] : 0.0;
#pragma unroll
  for (int j = 0; j < MU; j++) {
    if (j < nu) {
      x[j] = x[j] / Lf[j * ldl + j];
#pragma unroll
      for (int i = j + 1; i < MU; i++) if (i < nu) x[i] = fma(-Lf[i * ldl + j], x[j], x[i]);
    }
  }
#pragma unroll
  for (int j = MU - 1; j >= 0; j--) {
    if (j < nu) {
      x[j] = x[j] / Lf[j * ldl + j];
#pragma unroll
      for (int i = 0; i < j; i++) x[i] = fma(-Lf[j * ldl + i], x[j], x[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < MU; i++) if (i < nu) store(i, -x[i]);
}

// A pivot that is <= 0 or not finite at step t: reported, not propagated - zeros for the steps not solved and for the value terms,
// 1 + t in status
template <int NT>
MJB_LQR_DEV void lqr_report_pivot(const LqrBackwardArgs& p, int t, int e, int tid) {
  const int nx = p.nx, nu = p.nu;
  for (int s = 0; s <= t; s++) {
    double* ko = p.k + ((long)s * p.B + e) * nu;
    double* Ko = p.K + ((long)s * p.B + e) * nu * nx;
    for (int i = tid; i < nu; i += NT) ko[i] = 0.0;
    for (int i = tid; i < nu * nx; i += NT) Ko[i] = 0.0;
  }
  if (p.V0x) for (int i = tid; i < nx; i += NT) p.V0x[(long)e * nx + i] = 0.0;
  if (p.V0xx) for (int i = tid; i < nx * nx; i += NT) p.V0xx[(long)e * nx * nx + i] = 0.0;
  if (tid == 0) { p.dV[2 * e] = 0.0; p.dV[2 * e + 1] = 0.0; p.status[e] = 1 + t; }
}

// With R = [K | k]: S = Quu K + Qux, wq = Quu k; Vxx = Qxx + K^T S + Qux^T K (every lane reads and writes its own elements of Vxx),
// Vx = Qx + K^T (wq + Qu) + Qux^T k, and thread 0 adds the step's k^T Qu, k^T Quu k / 2 to dV1, dV2
template <int NW>
MJB_LQR_DEV void lqr_value_update(int nx, int nu, const LqrLds& m, int tid, double& dV1, double& dV2) {
  constexpr int NT = 64 * NW;
  const int ldr = nx + 1;
  double *Vxx = m.Vxx, *Vx = m.Vx, *Qux = m.Qux, *Quu = m.Quu, *Qx = m.Qx, *Qu = m.Qu, *wq = m.wq, *R = m.R, *S = m.S;
  lqr_gemm_tn<NW>(nu, nx, nu, Quu, nu, R, ldr, 0, nullptr, 0, nullptr, 0, tid, [&](int r, int c) { return Qux[r * nx + c]; },
                  [&](int r, int c, double v) { S[r * nx + c] = v; });
  for (int a = tid; a < nu; a += NT) {
    double s = 0.0;
    for (int b = 0; b < nu; b++) s = fma(Quu[a * nu + b], R[b * ldr + nx], s);
    wq[a] = s;
  }
  lqr_sync();

  lqr_gemm_tn<NW>(nx, nx, nu, R, ldr, S, nx, nu, Qux, nx, R, ldr, tid, [&](int r, int c) { return Vxx[r * nx + c]; },
                  [&](int r, int c, double v) { Vxx[r * nx + c] = v; });
  for (int i = tid; i < nx; i += NT) {
    double s = Qx[i];
    for (int a = 0; a < nu; a++) s = fma(R[a * ldr + i], wq[a] + Qu[a], s);
    for (int a = 0; a < nu; a++) s = fma(Qux[a * nx + i], R[a * ldr + nx], s);
    Vx[i] = s;
  }
  if (tid == 0) {
    double s1 = 0.0, s2 = 0.0;
    for (int a = 0; a < nu; a++) { s1 = fma(R[a * ldr + nx], Qu[a], s1); s2 = fma(R[a * ldr + nx], wq[a], s2); }
    dV1 += s1; dV2 += 0.5 * s2;
  }
  lqr_sync();
}

// Vxx <- (Vxx + Vxx^T) / 2, and the next step's blocks from the registers into LDS (K, S are no longer read)
template <int NT, int PA, int PB>
MJB_LQR_DEV void lqr_step_end(int nx, int nu, const LqrLds& m, int tid, const double (&ra)[PA], const double (&rb)[PB]) {
  double *Vxx = m.Vxx, *A = m.A, *Bt = m.B;
  for (int i = tid; i < nx * nx; i += NT) {
    const int r = i / nx, c = i % nx;
    if (c < r) { const double v = 0.5 * (Vxx[r * nx + c] + Vxx[c * nx + r]); Vxx[r * nx + c] = v; Vxx[c * nx + r] = v; }
  }
#pragma unroll
  for (int n = 0; n < PA; n++) { const int i = tid + n * NT; if (i < nx * nx) A[i] = ra[n]; }
#pragma unroll
  for (int n = 0; n < PB; n++) { const int i = tid + n * NT; if (i < nx * nu) Bt[i] = rb[n]; }
  lqr_sync();
}

// ---- the backward recursion of environment e ---------------------------------------------------------------------------------
// NW waves (64 NW threads, tid), nu <= MU (the unroll bound of the substitutions), w: the workgroup's LDS (lqr_layout(nx, nu).total doubles).
template <int NW, int MU>
MJB_LQR_DEV void lqr_backward_env(const LqrBackwardArgs& p, int e, int tid, double* w) {
  constexpr int NT = 64 * NW, PA = NW == 4 ? 16 : 4, PB = 8;     // PA, PB: elements of A_t, B_t one thread carries (nx <= 16 with one wave)
  const int nx = p.nx, nu = p.nu, T = p.T, ldr = nx + 1;
  const LqrLds m = lqr_lds_pointers(w, lqr_layout(nx, nu));
  double *R = m.R;
  const double mu = p.mu.p[(long)e * p.mu.es];
  double dV1 = 0.0, dV2 = 0.0;                                   // carried by thread 0
  lqr_load_terminal<NT>(p, e, m, tid);

  for (int t = T - 1; t >= 0; t--) {
    double ra[PA], rb[PB];
    lqr_prefetch<NT>(p, t, e, tid, ra, rb);
    lqr_step_products<NW>(p, t, e, mu, m, tid);

    // the solve's working set (it overlays A, B, VA, VB): Qw = Quu, R = [Qux | Qu]
    for (int i = tid; i < nu * nu; i += NT) m.Qw[i] = m.Quu[i];
    for (int i = tid; i < nu * ldr; i += NT) { const int a = i / ldr, c = i % ldr; R[i] = c < nx ? m.Qux[a * nx + c] : m.Qu[a]; }
    lqr_sync();
    if (!lqr_cholesky<NT>(m.Qw, m.L, nu, tid)) { lqr_report_pivot<NT>(p, t, e, tid); return; }

    // L L^T X = R, one thread per right-hand side: R <- -X = [K | k]
    double* ko = p.k + ((long)t * p.B + e) * nu;
    double* Ko = p.K + ((long)t * p.B + e) * nu * nx;
    for (int c = tid; c < ldr; c += NT)
      lqr_solve_column<MU>(R, ldr, m.L, nu, c, [&](int i, double v) {
        R[i * ldr + c] = v;
        if (c < nx) Ko[i * nx + c] = v; else ko[i] = v;
      });
    lqr_sync();

    lqr_value_update<NW>(nx, nu, m, tid, dV1, dV2);
    lqr_step_end<NT>(nx, nu, m, tid, ra, rb);
  }
  if (p.V0x) for (int i = tid; i < nx; i += NT) p.V0x[(long)e * nx + i] = m.Vx[i];
  if (p.V0xx) for (int i = tid; i < nx * nx; i += NT) p.V0xx[(long)e * nx * nx + i] = m.Vxx[i];
  if (tid == 0) { p.dV[2 * e] = dV1; p.dV[2 * e + 1] = dV2; p.status[e] = 0; }
}

// ---- the control-limited recursion of environment e (mjb_lqr_backward_box) ------------------------------------------------------
// Per step the box QP  min x' Quu x / 2 + Qu' x,  lob <= x <= hib  (lob = lo - u_t, hib = hi - u_t) by projected Newton (Tassa,
// Mansard, Todorov, ICRA 2014), then the step of lqr_backward_env with the clamped controls taken out of the solve.  The free block is
// never gathered: lqr_solve_face replaces the clamped rows and columns of Qw by identity and zeroes those rows of R, so the Cholesky
// and the substitution above run as they are, give on the free entries bitwise the compact factorisation, and with nothing clamped are
// the unconstrained arithmetic itself.  Every decision that encloses a barrier (the clamped set, feasibility, the trial accepted, a
// bad pivot) is read by every thread from the same LDS words after a barrier: workgroup-uniform.
MJB_LQR_DEV double lqr_clip(double v, double lo, double hi) { return v < lo ? lo : v > hi ? hi : v; }

template <int NW, int MU>
MJB_LQR_DEV void lqr_backward_box_env(const LqrBoxArgs& q, int e, int tid, double* w) {
  constexpr int NT = 64 * NW, PA = NW == 4 ? 16 : 4, PB = 8;
  const LqrBackwardArgs& p = q.b;
  const int nx = p.nx, nu = p.nu, T = p.T, ldr = nx + 1;
  const LqrBoxLay bl = lqr_box_layout(nx, nu);
  const LqrLds m = lqr_lds_pointers(w, bl.l);
  double *R = m.R, *Quu = m.Quu, *Qu = m.Qu;
  double *X = w + bl.x, *XS = w + bl.xs, *G = w + bl.g, *LOB = w + bl.lob, *HIB = w + bl.hib, *CF = w + bl.cf, *FE = w + bl.fe, *PASS = w + bl.pass;
  const unsigned full = nu >= 32 ? 0xffffffffu : (1u << nu) - 1u;
  const double mu = p.mu.p[(long)e * p.mu.es];
  const double lo_a = (q.lo && tid < nu) ? q.lo[tid] : -__builtin_huge_val();      // thread a < nu keeps the bounds of control a
  const double hi_a = (q.hi && tid < nu) ? q.hi[tid] : __builtin_huge_val();
  const double* ug = q.u.p + (long)e * q.u.es;
  double dV1 = 0.0, dV2 = 0.0;
  int failed = 0, itmax = 0;                                     // -(1 + t) of the highest step whose QP did not converge; the largest iteration count
  lqr_load_terminal<NT>(p, e, m, tid);

  // g = Qu + Quu x and the clamped set of x: (x == lob & g > 0) | (x == hib & g < 0), as a bit mask every thread holds
  auto clamped_set = [&]() -> unsigned {
    for (int a = tid; a < nu; a += NT) {
      double s = Qu[a];
      for (int b = 0; b < nu; b++) s = fma(Quu[a * nu + b], X[b], s);
      G[a] = s;
      CF[a] = ((X[a] == LOB[a] && s > 0.0) || (X[a] == HIB[a] && s < 0.0)) ? 1.0 : 0.0;
    }
    lqr_sync();
    unsigned c = 0;
    for (int a = 0; a < nu; a++) if (CF[a] != 0.0) c |= 1u << a;
    return c;
  };
  // R <- [K | k] of the face x_c = X_c: K_f, k_f = -Quu_ff^-1 [Qux_f | Qu_f + Quu_fc x_c], K_c = 0, k_c = x_c.  false at a bad pivot.
  auto solve_face = [&](unsigned c) -> bool {
    for (int i = tid; i < nu * nu; i += NT) {
      const int r = i / nu, cc = i % nu;
      m.Qw[i] = (((c >> r) | (c >> cc)) & 1u) ? (r == cc ? 1.0 : 0.0) : Quu[i];
    }
    for (int i = tid; i < nu * ldr; i += NT) {
      const int a = i / ldr, cc = i % ldr;
      double v = 0.0;
      if (!((c >> a) & 1u)) {
        if (cc < nx) v = m.Qux[a * nx + cc];
        else {
          v = Qu[a];
          for (int b = 0; b < nu; b++) if ((c >> b) & 1u) v = fma(Quu[a * nu + b], X[b], v);
        }
      }
      R[i] = v;
    }
    lqr_sync();
    if (!lqr_cholesky<NT>(m.Qw, m.L, nu, tid)) return false;
    for (int cc = tid; cc < ldr; cc += NT)
      lqr_solve_column<MU>(R, ldr, m.L, nu, cc, [&](int i, double v) { R[i * ldr + cc] = ((c >> i) & 1u) ? (cc < nx ? 0.0 : X[i]) : v; });
    lqr_sync();
    return true;
  };
  auto report_pivot = [&](int t) {
    lqr_report_pivot<NT>(p, t, e, tid);
    for (int s = tid; s <= t; s += NT) q.clamped[(long)s * p.B + e] = 0;
    if (tid == 0) q.qp_iters[e] = itmax;
  };

  for (int t = T - 1; t >= 0; t--) {
    double ra[PA], rb[PB];
    lqr_prefetch<NT>(p, t, e, tid, ra, rb);
    const double ru = tid < nu ? ug[(long)t * q.u.ss + tid] : 0.0;
    lqr_step_products<NW>(p, t, e, mu, m, tid);

    // the QP's box and starting point (they overlay A, B, VA, VB, as the solve's working set does): x = clip(0, lob, hib)
    if (tid < nu) {
      const double lob = lo_a - ru, hib = hi_a - ru;
      LOB[tid] = lob; HIB[tid] = hib; X[tid] = lqr_clip(0.0, lob, hib);
    }
    lqr_sync();
    unsigned c = clamped_set();
    int iters = 0;
    bool solved = false, stuck = false;                          // solved: R holds the face of the final set; stuck: a cap or a failed search
    for (;;) {
      iters++;
      if (c == full) break;                                      // no free control
      if (!solve_face(c)) { if (iters > itmax) itmax = iters; report_pivot(t); return; }
      // the Newton target x* (a point, not an increment): taken whole when it lies in the box
      if (tid < nu) {
        const double v = R[tid * ldr + nx];
        XS[tid] = v;
        FE[tid] = lqr_clip(v, LOB[tid], HIB[tid]) == v ? 1.0 : 0.0;
      }
      lqr_sync();
      bool inside = true;
      for (int a = 0; a < nu; a++) if (FE[a] == 0.0) inside = false;
      if (inside) {
        if (tid < nu) X[tid] = XS[tid];
        lqr_sync();
        const unsigned c2 = clamped_set();
        if (c2 == c) { solved = true; break; }                   // the same set at x*: done, tolerance-free
        c = c2;
      } else {
        // Armijo search on clip(x + s (x* - x)), s = 0.6^j: trial j on thread j, the first that passes is the serial search's
        if (tid < kLqrQpTrials) {
          double sdotg = 0.0, fold = 0.0, fnew = 0.0, s = 1.0;
          for (int j = 0; j < tid; j++) s *= 0.6;
          for (int a = 0; a < nu; a++) sdotg = fma(G[a], XS[a] - X[a], sdotg);
          for (int a = 0; a < nu; a++) {
            double h0 = 0.0, h1 = 0.0;
            for (int b = 0; b < nu; b++) {
              const double yb = lqr_clip(X[b] + s * (XS[b] - X[b]), LOB[b], HIB[b]);
              h0 = fma(Quu[a * nu + b], X[b], h0); h1 = fma(Quu[a * nu + b], yb, h1);
            }
            const double ya = lqr_clip(X[a] + s * (XS[a] - X[a]), LOB[a], HIB[a]);
            fold = fma(X[a], Qu[a] + 0.5 * h0, fold); fnew = fma(ya, Qu[a] + 0.5 * h1, fnew);
          }
          PASS[tid] = (sdotg < 0.0 && fnew - fold <= 0.1 * s * sdotg) ? 1.0 : 0.0;
        }
        lqr_sync();
        int first = -1;
        for (int j = kLqrQpTrials - 1; j >= 0; j--) if (PASS[j] != 0.0) first = j;
        if (first < 0) { stuck = true; break; }                  // the search failed: keep the iterate
        if (tid < nu) {
          double s = 1.0;
          for (int j = 0; j < first; j++) s *= 0.6;
          X[tid] = lqr_clip(X[tid] + s * (XS[tid] - X[tid]), LOB[tid], HIB[tid]);
        }
        lqr_sync();
        c = clamped_set();
      }
      if (iters == kLqrQpIters) { stuck = true; break; }
    }
    if (iters > itmax) itmax = iters;
    if (stuck && !failed) failed = -(1 + t);
    // the polish: one solve on the final set (already in R when the QP ended on it), k = clip(k, lob, hib)
    if (!solved && !solve_face(c)) { report_pivot(t); return; }
    double* ko = p.k + ((long)t * p.B + e) * nu;
    double* Ko = p.K + ((long)t * p.B + e) * nu * nx;
    if (tid < nu) {
      const double v = lqr_clip(R[tid * ldr + nx], LOB[tid], HIB[tid]);
      R[tid * ldr + nx] = v; ko[tid] = v;
    }
    for (int i = tid; i < nu * nx; i += NT) Ko[i] = R[(i / nx) * ldr + i % nx];
    if (tid == 0) q.clamped[(long)t * p.B + e] = (int)c;
    lqr_sync();

    lqr_value_update<NW>(nx, nu, m, tid, dV1, dV2);
    lqr_step_end<NT>(nx, nu, m, tid, ra, rb);
  }
  if (p.V0x) for (int i = tid; i < nx; i += NT) p.V0x[(long)e * nx + i] = m.Vx[i];
  if (p.V0xx) for (int i = tid; i < nx * nx; i += NT) p.V0xx[(long)e * nx * nx + i] = m.Vxx[i];
  if (tid == 0) { p.dV[2 * e] = dV1; p.dV[2 * e + 1] = dV2; p.status[e] = failed; q.qp_iters[e] = itmax; }
}

// ---- the candidate controls of environment e, every step size --------------------------------------------------------------
// c_t = clamp(u_t + alpha_j k_t + K_t dx, lo, hi), dx <- A_t dx + B_t (c_t - u_t); NT threads, mat-vecs only: the step's blocks are
// staged once in LDS and every step size reads them there.
template <int NT>
MJB_LQR_DEV void lqr_candidates_env(const LqrCandArgs& p, int e, int tid, double* w) {
  const int nx = p.nx, nu = p.nu, na = p.nalpha, T = p.T;
  const LqrCandLay l = lqr_cand_layout(nx, nu, na);
  const int lda = l.lda;
  double *A = w + l.A, *Bt = w + l.B, *K = w + l.K, *kv = w + l.k, *uv = w + l.u, *du = w + l.du;
  double *dx = w + l.dx, *dxn = w + l.dx + na * nx;
  for (int i = tid; i < na * nx; i += NT) dx[i] = p.dx0.p ? p.dx0.p[(long)e * p.dx0.es + i % nx] : 0.0;
  for (int t = 0; t < T; t++) {
    const double* Ag = p.A.p + (long)t * p.A.ss + (long)e * p.A.es;
    const double* Bg = p.Bm.p + (long)t * p.Bm.ss + (long)e * p.Bm.es;
    const double* Kg = p.K.p + (long)t * p.K.ss + (long)e * p.K.es;
    const double* kg = p.k.p + (long)t * p.k.ss + (long)e * p.k.es;
    const double* ug = p.u.p + (long)t * p.u.ss + (long)e * p.u.es;
    for (int i = tid; i < nx * nx; i += NT) A[(i / nx) * lda + i % nx] = Ag[i];
    for (int i = tid; i < nu * nx; i += NT) K[(i / nx) * lda + i % nx] = Kg[i];
    for (int i = tid; i < nx * nu; i += NT) Bt[i] = Bg[i];
    for (int i = tid; i < nu; i += NT) { kv[i] = kg[i]; uv[i] = ug[i]; }
    lqr_sync();
    for (int i = tid; i < na * nu; i += NT) {
      const int j = i / nu, a = i % nu;
      double s = 0.0;
      for (int x = 0; x < nx; x++) s = fma(K[a * lda + x], dx[j * nx + x], s);
      double c = uv[a] + p.alphas[j] * kv[a] + s;
      if (p.lo && c < p.lo[a]) c = p.lo[a];
      if (p.hi && c > p.hi[a]) c = p.hi[a];
      du[i] = c - uv[a];
      const long o = (((long)e * na + j) * T + t) * nu + a;
      if (p.out_f32) ((float*)p.cand)[o] = (float)c; else ((double*)p.cand)[o] = c;
    }
    lqr_sync();
    for (int i = tid; i < na * nx; i += NT) {
      const int j = i / nx, r = i % nx;
      double s = 0.0;
      for (int x = 0; x < nx; x++) s = fma(A[r * lda + x], dx[j * nx + x], s);
      for (int a = 0; a < nu; a++) s = fma(Bt[r * nu + a], du[j * nu + a], s);
      dxn[i] = s;
    }
    lqr_sync();
    double* sw = dx; dx = dxn; dxn = sw;
  }
}

#ifndef MJB_HOST_EMU
// enqueue only (mjb_lqr.hip); the entry points (mjb_api.hip) have checked every pointer and extent
hipError_t lqr_launch_backward(const LqrBackwardArgs& p, hipStream_t stream);
hipError_t lqr_launch_backward_box(const LqrBoxArgs& p, hipStream_t stream);
hipError_t lqr_launch_candidates(const LqrCandArgs& p, hipStream_t stream);
hipError_t lqr_launch_gemm_probe(int M, int N, int K, const double* a, const double* b, double* c, hipStream_t stream);
#endif

}  // namespace mjb
