// vcmpc_abi.hip -- the C ABI of libvcmpc.so (declared in include/vcmpc.h).
//
// Context management, argument validation, host<->device staging for
// VC_HOST_PTRS calls, and dispatch to the HIP kernels.  No compute happens on
// the host: every numeric result comes from a gfx950 kernel.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "vc_kernels.hpp"
#include "vcmpc.h"


// In-kernel infeasibility detection (vc_set_infeasibility / vc_set_sqp_infeasibility /
// vc_set_casc_infeasibility) and the Farkas certificates of the last solve.
struct Detect {
  bool on = false;
  double eps = 1e-9;
  void* farkas = nullptr;    // [max_batch][rows] fp64, allocated on first enable, kept when turned off
  void* qp_index = nullptr;  // [max_batch] int32, the SQP models only
  size_t rows = 0;           // per problem: 7N-3 (kinematic), 12N-3 (single track), 12N-3+6M (cascaded)
  int B = 0;                 // batch of the last solve that wrote them
};

// Regularised retry of the single-track SQP's QPs (vc_set_sqp_regularization), the levels of the
// last solve and the breakdown test hook (vc_debug_sqp_breakdown).
struct Regularize {
  int levels = 0;            // 0: off
  double factor = 10.0;
  void* level = nullptr;     // [B][sqp_iters] int32 of the last solve (grow-only scratch)
  size_t level_bytes = 0;
  int B = 0, K = 0;          // batch and sqp_iters of the last solve that wrote it
  int dbg_sqp_iter = -1, dbg_problem = -1, dbg_levels = 0;
};

struct vc_ctx {
  int device = 0, model = 0, N = 0, max_batch = 0, dtype = 0;
  vc_params p{};
  hipStream_t own = nullptr;
  hipStream_t stream = nullptr;
  void* arena = nullptr;
  size_t arena_bytes = 0;
  void* track = nullptr;  // vc_track_set: [n][4] fp64 curvature pieces
  int track_n = 0;
  double track_h = 0.0, track_len = 0.0;
  void* sim = nullptr;    // vc_simulate scratch (kappa, ds, x, u0, status, iters)
  size_t sim_bytes = 0;
  void* ls = nullptr;     // kinematic SQP scratch (vc_qp.kin_sqp > 0): u_prev, status / iteration sums
  size_t ls_bytes = 0;
  void* jw = nullptr;     // single-track / cascaded SQP: stage Jacobians of the kernels that keep them out of LDS
  size_t jw_bytes = 0;
  int fault_iter = -1, fault_problem = -1;  // vc_debug_qp_fault (tests only)
  Detect det;             // vc_set_*_infeasibility (a context has one model, so one state)
  Regularize reg;         // vc_set_sqp_regularization / vc_debug_sqp_breakdown (single-track fp64 SQP)
  std::string err;
};

namespace {
thread_local std::string g_create_err;

int fail(vc_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  else g_create_err = buf;
  return code;
}

#define VC_HIP(ctx, call)                                                                         \
  do {                                                                                            \
    hipError_t e_ = (call);                                                                       \
    if (e_ != hipSuccess) return fail((ctx), VC_E_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
  } while (0)

size_t esize(const vc_ctx* c) { return c->dtype == VC_F32 ? 4 : 8; }

// Grow-only device scratch owned by the context (freed once the stream has drained).
int ensure_scratch(vc_ctx* c, void** p, size_t* have, size_t need) {
  if (need <= *have) return 0;
  VC_HIP(c, hipStreamSynchronize(c->stream));
  if (*p) VC_HIP(c, hipFree(*p));
  *p = nullptr;
  *have = 0;
  VC_HIP(c, hipMalloc(p, need));
  *have = need;
  return 0;
}
int nx_of(const vc_ctx* c) { return c->model == VC_MODEL_KINEMATIC ? 6 : 8; }

int ensure_arena(vc_ctx* c, size_t bytes) {
  if (bytes <= c->arena_bytes) return 0;
  VC_HIP(c, hipSetDevice(c->device));
  if (c->arena) VC_HIP(c, hipFree(c->arena));
  c->arena = nullptr;
  c->arena_bytes = 0;
  VC_HIP(c, hipMalloc(&c->arena, bytes));
  c->arena_bytes = bytes;
  return 0;
}

size_t al256(size_t b) { return (b + 255) & ~size_t(255); }

// A device pointer of whatever element type and constness the kernel's argument wants.
struct Ptr {
  void* p = nullptr;
  template <class T> operator T*() const { return static_cast<T*>(p); }
};

// The buffers of one entry-point call.  Each is declared once, inside the callable given to bind(),
// and the declaration returns the pointer for the kernel: the caller's own under VC_DEVICE_PTRS
// (no copy, no synchronise), a 256-byte-aligned arena slice under VC_HOST_PTRS.  There bind() runs
// the declarations twice: first to add the sizes up, so the arena grows at most once and before any
// copy, then to hand out the slices and issue the H2D copies in declaration order.  After the
// launches finish() issues the D2H copies and synchronises once.  An optional buffer passed as NULL
// takes no bytes and reaches the kernel as nullptr in both modes.
class Staging {
 public:
  Staging(vc_ctx* c, int flags) : c_(c), host_(flags == VC_HOST_PTRS) {}

  struct Pair {
    Ptr rd, wr;  // what the kernel reads / writes; null where src / dst is
  };
  // one slice copied in from src (if any) and back out to dst (if any)
  Pair pair(const void* src, void* dst, size_t bytes) {
    if (!host_) return {{const_cast<void*>(src)}, {dst}};
    if (!src && !dst) return {};
    const size_t at = off_;
    off_ += al256(bytes);
    if (!placing_) return {};
    void* dev = static_cast<char*>(c_->arena) + at;
    if (src && bytes && err_ == hipSuccess) err_ = hipMemcpyAsync(dev, src, bytes, hipMemcpyHostToDevice, c_->stream);
    if (dst && bytes) outs_.push_back({dst, dev, bytes});
    return {{src ? dev : nullptr}, {dst ? dev : nullptr}};
  }
  Ptr in(const void* host, size_t bytes) { return pair(host, nullptr, bytes).rd; }
  Ptr out(void* host, size_t bytes) { return pair(nullptr, host, bytes).wr; }
  Ptr inout(void* host, size_t bytes) { return pair(host, host, bytes).wr; }

  template <class F>
  int bind(F&& declare) {
    declare();
    if (!host_) return 0;
    if (int r = ensure_arena(c_, off_ ? off_ : 256)) return r;
    off_ = 0;
    placing_ = true;
    declare();
    if (err_ != hipSuccess) return fail(c_, VC_E_HIP, "hipMemcpyAsync (H2D): %s", hipGetErrorString(err_));
    return 0;
  }

  int finish() {
    if (!host_) return 0;
    for (const Out& o : outs_) VC_HIP(c_, hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, c_->stream));
    VC_HIP(c_, hipStreamSynchronize(c_->stream));
    return 0;
  }

 private:
  struct Out {
    void* host;
    const void* dev;
    size_t bytes;
  };
  vc_ctx* c_;
  bool host_, placing_ = false;
  size_t off_ = 0;
  hipError_t err_ = hipSuccess;
  std::vector<Out> outs_;
};

int check_common(vc_ctx* c, int B, int flags) {
  if (!c) return VC_E_ARG;
  if (B < 0 || B > c->max_batch) return fail(c, VC_E_ARG, "batch %d outside [0, max_batch=%d]", B, c->max_batch);
  if (flags != VC_HOST_PTRS && flags != VC_DEVICE_PTRS) return fail(c, VC_E_ARG, "bad flags %d", flags);
  hipError_t e = hipSetDevice(c->device);
  if (e != hipSuccess) return fail(c, VC_E_HIP, "hipSetDevice: %s", hipGetErrorString(e));
  return 0;
}

vc::ModelArgs model_args(const vc_ctx* c, int B) {
  vc::ModelArgs m{};
  m.model = c->model;
  m.B = B;
  m.N = c->N;
  m.M = c->model == VC_MODEL_CASCADED ? c->p.casc.horizon_pm : 0;
  m.shift = c->p.qp.shift;
  m.L = c->p.kin_car.l;
  m.dyn64 = vc::make_dyn_coef<double>(c->p.dyn_car);
  m.dyn32 = vc::make_dyn_coef<float>(c->p.dyn_car);
  return m;
}

// stages of the solve arrays: kappa / ds / ubar span H (= N, or N + horizon_pm for a
// cascaded context); xbar has N + 1 (kinematic) or H state columns
int nh_of(const vc_ctx* c) { return c->N + (c->model == VC_MODEL_CASCADED ? c->p.casc.horizon_pm : 0); }
int ns_of(const vc_ctx* c) { return c->model == VC_MODEL_KINEMATIC ? c->N + 1 : nh_of(c); }
vc::TrackTable track_table(const vc_ctx* c) {
  return vc::TrackTable{static_cast<const double*>(c->track), c->track_n, c->track_h, c->track_len};
}

// The condensed kernel (kin_ltv.hip) where it is built (N = 20, the bench's C2/C4 shape),
// the stagewise Riccati kernel (kin_ric.hip) for the other horizons (kinematic.yaml: 50).
// the condensed kernel for the one-step contract only: the globalised step's QPs (obstacle
// barriers, condition numbers ~1e6) need the stagewise factorisation's accuracy (kin_ric.hip
// matches the oracle to 1e-8 there, the condensed normal equations to 8e-5; scripts/kin_sqp_debug.py)
bool kin_condensed_cfg(const vc_ctx* c) {
  // elastic rows (qp.elastic) and multiple shooting are built in the stagewise kernel only
  // (qp.solver = 2: as 0, with the infeasibility detection inside the condensed kernel -- below)
  return vc::kin_ltv_smem_bytes(c->N) > 0 && (c->p.qp.solver == 0 || c->p.qp.solver == 2) && c->p.qp.kin_sqp <= 0 &&
         !c->p.qp.ms && c->p.qp.elastic == 0.0;
}
// The infeasibility detection (vc_set_infeasibility) is built in both kernels.  On a qp.solver = 0
// context the solve of a context that has it on goes to the stagewise kernel (the routing since ABI 13);
// qp.solver = 2 keeps the condensed kernel and its DET instantiation runs the test (kin_ltv.hip).
// vc_condense keeps the condensed kernel's H, g either way.
bool kin_condensed(const vc_ctx* c) { return kin_condensed_cfg(c) && (!c->det.on || c->p.qp.solver == 2); }
bool kin_solve_built(const vc_ctx* c) {
  return c->model == VC_MODEL_KINEMATIC && c->dtype == VC_F64 && (kin_condensed(c) || vc::kin_ric_built(c->N));
}
bool dyn_solve_built(const vc_ctx* c) {
  if (c->model != VC_MODEL_DYNAMIC) return false;
  if (c->dtype == VC_F32) return vc::dyn_sqp_smem_bytes(c->N) > 0;
  return vc::st_sqp_built(c->N);
}
// Cascaded: the stagewise Riccati kernel (casc_ric.hip; M = 15, 25, 35, 40) unless
// qp.solver = 2 asks for the condensed one (casc_sqp.hip, M = 40).
bool casc_stagewise(const vc_ctx* c) {
  return c->p.qp.solver != 2 && vc::casc_ric_built(c->N, c->p.casc.horizon_pm);
}
bool casc_solve_built(const vc_ctx* c) {
  return c->model == VC_MODEL_CASCADED && c->dtype == VC_F64 &&
         (casc_stagewise(c) || vc::casc_sqp_built(c->N, c->p.casc.horizon_pm));
}

// vc_set_*_infeasibility behind its entry point's own "supported here" checks: the certificate
// buffers are sized by max_batch on first enable and kept until vc_destroy.
int set_detection(vc_ctx* c, int on, double eps, size_t rows, bool with_index) {
  Detect& d = c->det;
  if (on && !d.farkas) {
    VC_HIP(c, hipSetDevice(c->device));
    const size_t nb = (size_t)(c->max_batch > 0 ? c->max_batch : 1);
    VC_HIP(c, hipMalloc(&d.farkas, nb * rows * 8));
    if (with_index) VC_HIP(c, hipMalloc(&d.qp_index, nb * 4));
  }
  d.on = on != 0;
  d.eps = eps > 0.0 ? eps : 1e-9;
  d.rows = rows;
  d.B = 0;  // no solve has written certificates under this setting yet
  return 0;
}

// vc_get_*_farkas of the entry point `who`, which serves contexts of `model`: on any other context
// its detection is off by definition.
int get_detection(vc_ctx* c, const char* who, int model, int B, void* y, int32_t* qp_index, bool with_index,
                  int flags) {
  if (int r = check_common(c, B, flags)) return r;
  const Detect& d = c->det;
  if (c->model != model || !d.on || !d.farkas || (with_index && !d.qp_index))
    return fail(c, VC_E_ARG, "%s: infeasibility detection is off", who);
  if (model == VC_MODEL_KINEMATIC && c->p.qp.kin_sqp > 0)
    return fail(c, VC_E_UNSUPPORTED, "%s: kin_sqp > 0 solves several QPs per call", who);
  if (B > d.B) return fail(c, VC_E_ARG, "%s: B=%d exceeds the last solve's %d", who, B, d.B);
  if (!y) return fail(c, VC_E_ARG, "null pointer");
  if (B == 0) return 0;
  const hipMemcpyKind kind = flags == VC_DEVICE_PTRS ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  VC_HIP(c, hipMemcpyAsync(y, d.farkas, (size_t)B * d.rows * 8, kind, c->stream));
  if (qp_index) VC_HIP(c, hipMemcpyAsync(qp_index, d.qp_index, (size_t)B * 4, kind, c->stream));
  if (flags != VC_DEVICE_PTRS) VC_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

// The detect / detect_eps / farkas tail of a solve kernel's arguments; true when the detection is on
// (the SQP kernels then take qp_index too).
template <class Args>
bool arm_detection(vc_ctx* c, Args& a, int B) {
  if (!c->det.on) return false;
  a.detect = 1;
  a.detect_eps = c->det.eps;
  a.farkas = (double*)c->det.farkas;
  c->det.B = B;
  return true;
}

// The reg_* / level / dbg_* tail of the single-track SQP kernel's arguments: the ladder where it is on
// (the level buffer sized for this launch), the test hook where it is armed.
int arm_regularization(vc_ctx* c, vc::StSqpArgs& a, int B) {
  Regularize& r = c->reg;
  if (r.levels > 0) {
    const int K = c->p.dyn_mpc.sqp_iters;
    if (int e = ensure_scratch(c, &r.level, &r.level_bytes, (size_t)B * K * 4)) return e;
    a.reg_levels = r.levels;
    a.reg_factor = r.factor;
    a.level = (int32_t*)r.level;
    r.B = B;
    r.K = K;
  }
  if (r.dbg_sqp_iter >= 0 && r.dbg_levels > 0) {
    a.dbg_levels = r.dbg_levels;
    a.dbg_sqp_iter = r.dbg_sqp_iter;
    a.dbg_problem = r.dbg_problem;
  }
  return 0;
}

// Cascaded single-track + point-mass SQP (casc_sqp.hip), fp64: arrays span H = N + M stages.
// mode 0: solve (xbar, ubar, u0, status, iters, diag); mode 1: first QP's H, g (H_out, g_out).
int casc_solve(vc_ctx* c, int B, const void* x0, const void* kappa, const void* ds, void* xbar, void* ubar, void* u0,
               int32_t* status, int32_t* iters, void* diag, int flags, int mode = 0, void* H_out = nullptr,
               void* g_out = nullptr) {
  const int Hs = c->N + c->p.casc.horizon_pm, n = 2 * Hs, nx = 8, nu = 2;
  const vc_dyn_mpc& w = c->p.dyn_mpc;
  if (w.sqp_iters < 1 || w.sqp_iters > 64) return fail(c, VC_E_ARG, "dyn_mpc.sqp_iters=%d outside [1,64]", w.sqp_iters);
  if (!(w.fx_scale > 0)) return fail(c, VC_E_ARG, "dyn_mpc.fx_scale must be > 0");
  if (c->p.qp.max_iter < 1) return fail(c, VC_E_ARG, "qp.max_iter must be >= 1");
  if (!(c->p.casc.ds_pm > 0)) return fail(c, VC_E_ARG, "casc.ds_pm must be > 0");
  vc::CascSqpArgs a{};
  a.B = B;
  a.mode = mode;
  a.car = vc::make_dyn_coef<double>(c->p.dyn_car);
  a.w = w;
  a.cw = c->p.casc;
  a.qp = c->p.qp;
  a.obs = c->p.obs;
  Staging st(c, flags);
  if (int r = st.bind([&] {
        a.x0 = st.in(x0, (size_t)B * nx * 8);
        a.kappa = st.in(kappa, (size_t)B * Hs * 8);
        a.ds = st.in(ds, (size_t)B * Hs * 8);
        // mode 1 reads the warm start only: ubar is not written back
        const Staging::Pair u = st.pair(ubar, mode == 0 ? ubar : nullptr, (size_t)B * Hs * nu * 8);
        a.ubar = u.rd;
        a.u_out = u.wr;
        if (mode == 0) {
          a.x_out = st.out(xbar, (size_t)B * Hs * nx * 8);
          a.u0 = st.out(u0, (size_t)B * nu * 8);
          a.status = st.out(status, (size_t)B * 4);
          a.iters = st.out(iters, (size_t)B * 4);
          a.diag = st.out(diag, (size_t)B * VC_CASC_DIAG_COLS * 8);
        } else {
          a.H_out = st.out(H_out, (size_t)B * n * n * 8);
          a.g_out = st.out(g_out, (size_t)B * n * 8);
        }
      }))
    return r;
  if (mode == 0 && casc_stagewise(c)) {
    if (const size_t jd = vc::casc_ric_jws_doubles(c->N, c->p.casc.horizon_pm, B)) {
      if (int r = ensure_scratch(c, &c->jw, &c->jw_bytes, (size_t)B * jd * 8)) return r;
      a.jws = (double*)c->jw;
    }
    if (arm_detection(c, a, B)) a.qp_index = (int32_t*)c->det.qp_index;
    VC_HIP(c, vc::launch_casc_ric(a, c->N, c->p.casc.horizon_pm, c->stream));
  }
  else VC_HIP(c, vc::launch_casc_sqp(a, c->N, c->p.casc.horizon_pm, c->stream));
  return st.finish();
}

// Dynamic single-track SQP, fp64 (st_sqp.hip, stagewise Riccati interior point): xbar has
// N state columns.
int st_solve(vc_ctx* c, int B, const void* x0, const void* kappa, const void* ds, void* xbar, void* ubar, void* u0,
             int32_t* status, int32_t* iters, void* diag, int flags) {
  const int N = c->N, nx = 8, nu = 2;
  const vc_dyn_mpc& w = c->p.dyn_mpc;
  vc::StSqpArgs a{};
  a.B = B;
  a.car = vc::make_dyn_coef<double>(c->p.dyn_car);
  a.w = w;
  a.qp = c->p.qp;
  a.obs = c->p.obs;
  Staging st(c, flags);
  if (int r = st.bind([&] {
        a.x0 = st.in(x0, (size_t)B * nx * 8);
        a.kappa = st.in(kappa, (size_t)B * N * 8);
        a.ds = st.in(ds, (size_t)B * N * 8);
        a.ubar = a.u_out = st.inout(ubar, (size_t)B * N * nu * 8);
        a.x_out = st.out(xbar, (size_t)B * N * nx * 8);
        a.u0 = st.out(u0, (size_t)B * nu * 8);
        a.status = st.out(status, (size_t)B * 4);
        a.iters = st.out(iters, (size_t)B * 4);
        a.diag = st.out(diag, (size_t)B * VC_ST_DIAG_COLS * 8);
      }))
    return r;
  if (const size_t jd = vc::st_sqp_jws_doubles(N, B)) {
    if (int r = ensure_scratch(c, &c->jw, &c->jw_bytes, (size_t)B * jd * 8)) return r;
    a.jws = (double*)c->jw;
  }
  if (arm_detection(c, a, B)) a.qp_index = (int32_t*)c->det.qp_index;
  if (int r = arm_regularization(c, a, B)) return r;
  VC_HIP(c, vc::launch_st_sqp(a, N, c->stream));
  return st.finish();
}

// Dynamic single-track SQP (dyn_sqp.hip), fp32: xbar has N state columns.
int dyn_solve(vc_ctx* c, int B, const void* x0, const void* kappa, const void* ds, void* xbar, void* ubar, void* u0,
              int32_t* status, int32_t* iters, void* diag, int flags, void* dbg = nullptr) {
  const int N = c->N, nx = 8, nu = 2;
  const vc_dyn_mpc& w = c->p.dyn_mpc;
  if (w.sqp_iters < 1 || w.sqp_iters > 64) return fail(c, VC_E_ARG, "dyn_mpc.sqp_iters=%d outside [1,64]", w.sqp_iters);
  if (!(w.fx_scale > 0)) return fail(c, VC_E_ARG, "dyn_mpc.fx_scale must be > 0");
  if (c->p.qp.max_iter < 1) return fail(c, VC_E_ARG, "qp.max_iter must be >= 1");
  if (c->dtype == VC_F64) return st_solve(c, B, x0, kappa, ds, xbar, ubar, u0, status, iters, diag, flags);
  vc::DynSqpArgs a{};
  a.B = B;
  a.car = vc::make_dyn_coef<float>(c->p.dyn_car);
  a.w = w;
  a.qp = c->p.qp;
  a.obs = c->p.obs;
  Staging st(c, flags);
  if (int r = st.bind([&] {
        a.x0 = st.in(x0, (size_t)B * nx * 4);
        a.kappa = st.in(kappa, (size_t)B * N * 4);
        a.ds = st.in(ds, (size_t)B * N * 4);
        a.ubar = a.u_out = st.inout(ubar, (size_t)B * N * nu * 4);
        a.x_out = st.out(xbar, (size_t)B * N * nx * 4);
        a.u0 = st.out(u0, (size_t)B * nu * 4);
        a.status = st.out(status, (size_t)B * 4);
        a.iters = st.out(iters, (size_t)B * 4);
        a.diag = st.out(diag, (size_t)B * VC_DYN_DIAG_COLS * 4);
        a.dbg = st.out(dbg, (size_t)B * vc::dyn_sqp_debug_stride() * 4);
      }))
    return r;
  VC_HIP(c, vc::launch_dyn_sqp(a, N, c->stream));
  return st.finish();
}
}  // namespace

extern "C" {

int vc_abi_version(void) { return VCMPC_ABI_VERSION; }
int vc_params_sizeof(void) { return (int)sizeof(vc_params); }

// Shared by vc_create and vc_set_obstacles: NULL when the set is usable, else the reason.
static const char* obstacles_invalid(const vc_obstacles& o) {
  static thread_local char msg[96];
  if (o.n < 0 || o.n > VC_MAX_OBSTACLES) {
    snprintf(msg, sizeof msg, "n=%d obstacles outside [0,%d]", o.n, VC_MAX_OBSTACLES);
    return msg;
  }
  for (int j = 0; j < o.n; ++j)
    if (!std::isfinite(o.s[j]) || !std::isfinite(o.ey[j]) || !std::isfinite(o.radius[j])) {
      snprintf(msg, sizeof msg, "obstacle %d is not finite", j);
      return msg;
    }
  return nullptr;
}

vc_ctx* vc_create(int device, int model, int N, int max_batch, int dtype, const vc_params* params) {
  g_create_err.clear();
  if (!params) { fail(nullptr, VC_E_ARG, "params is NULL"); return nullptr; }
  if (model != VC_MODEL_KINEMATIC && model != VC_MODEL_DYNAMIC && model != VC_MODEL_CASCADED) {
    fail(nullptr, VC_E_ARG, "bad model %d", model);
    return nullptr;
  }
  if (model == VC_MODEL_CASCADED && (params->casc.horizon_pm < 1 || params->casc.horizon_pm > 4096)) {
    fail(nullptr, VC_E_ARG, "cascaded context needs casc.horizon_pm >= 1 (got %d)", params->casc.horizon_pm);
    return nullptr;
  }
  if (dtype != VC_F64 && dtype != VC_F32) { fail(nullptr, VC_E_ARG, "bad dtype %d", dtype); return nullptr; }
  if (N < 1 || N > 4096) { fail(nullptr, VC_E_ARG, "bad horizon N=%d", N); return nullptr; }
  if (max_batch < 1) { fail(nullptr, VC_E_ARG, "bad max_batch %d", max_batch); return nullptr; }
  // obs.inside (ABI 11) is a switch, and only the SQP models' QP and merit use it: the kinematic
  // merit keeps its C1 extension inside the margin floor, so an inside-mode kinematic QP would
  // disagree with its own line search
  if (params->obs.inside != 0 && params->obs.inside != 1) {
    fail(nullptr, VC_E_ARG, "obs.inside=%d must be 0 or 1", params->obs.inside);
    return nullptr;
  }
  if (model == VC_MODEL_KINEMATIC && params->obs.inside) {
    fail(nullptr, VC_E_ARG, "obs.inside=1 is not supported by the kinematic model (dynamic / cascaded only)");
    return nullptr;
  }
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0) {
    fail(nullptr, VC_E_HIP, "no HIP device available (%s)", hipGetErrorString(e));
    return nullptr;
  }
  if (device < 0 || device >= ndev) { fail(nullptr, VC_E_ARG, "device %d not in [0,%d)", device, ndev); return nullptr; }
  e = hipSetDevice(device);
  if (e != hipSuccess) { fail(nullptr, VC_E_HIP, "hipSetDevice: %s", hipGetErrorString(e)); return nullptr; }
  // the obstacle set is validated by the same rule as vc_set_obstacles, before any allocation
  if (const char* why = obstacles_invalid(params->obs)) {
    fail(nullptr, VC_E_ARG, "params->obs: %s", why);
    return nullptr;
  }
  vc_ctx* c = new vc_ctx();
  c->device = device;
  c->model = model;
  c->N = N;
  c->max_batch = max_batch;
  c->dtype = dtype;
  c->p = *params;
  if (!(c->p.obs.margin_min > 0)) c->p.obs.margin_min = VC_OBS_MARGIN_MIN;
  e = hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking);
  if (e != hipSuccess) {
    fail(nullptr, VC_E_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
    delete c;
    return nullptr;
  }
  c->stream = c->own;
  return c;
}

void vc_destroy(vc_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->arena) (void)hipFree(c->arena);
  if (c->track) (void)hipFree(c->track);
  if (c->sim) (void)hipFree(c->sim);
  if (c->ls) (void)hipFree(c->ls);
  if (c->jw) (void)hipFree(c->jw);
  if (c->det.farkas) (void)hipFree(c->det.farkas);
  if (c->det.qp_index) (void)hipFree(c->det.qp_index);
  if (c->reg.level) (void)hipFree(c->reg.level);
  if (c->own) (void)hipStreamDestroy(c->own);
  delete c;
}

const char* vc_last_error(const vc_ctx* c) { return c ? c->err.c_str() : g_create_err.c_str(); }

int vc_set_stream(vc_ctx* c, void* stream) {
  if (!c) return VC_E_ARG;
  c->stream = stream ? static_cast<hipStream_t>(stream) : c->own;
  return 0;
}

int vc_set_obstacles(vc_ctx* c, int n, const double* s, const double* ey, const double* radius, double margin_min) {
  if (!c) return VC_E_ARG;
  if (n < 0 || n > VC_MAX_OBSTACLES) return fail(c, VC_E_ARG, "n=%d obstacles outside [0,%d]", n, VC_MAX_OBSTACLES);
  if (n > 0 && (!s || !ey || !radius)) return fail(c, VC_E_ARG, "null pointer");
  vc_obstacles o{};
  o.n = n;
  o.inside = c->p.obs.inside;  // the barrier mode is the context's (vc_create's params)
  o.margin_min = margin_min > 0 ? margin_min : c->p.obs.margin_min;
  for (int j = 0; j < n; ++j) {
    o.s[j] = s[j];
    o.ey[j] = ey[j];
    o.radius[j] = radius[j];
  }
  if (const char* why = obstacles_invalid(o)) return fail(c, VC_E_ARG, "%s", why);
  c->p.obs = o;
  return 0;
}

int vc_synchronize(vc_ctx* c) {
  if (!c) return VC_E_ARG;
  VC_HIP(c, hipSetDevice(c->device));
  VC_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

int vc_set_infeasibility(vc_ctx* c, int on, double eps) {
  if (!c) return VC_E_ARG;
  if (c->model != VC_MODEL_KINEMATIC || c->dtype != VC_F64 || !vc::kin_ric_built(c->N))
    return fail(c, VC_E_UNSUPPORTED,
                "vc_set_infeasibility: the stagewise kinematic kernel only (kinematic fp64, N=10..60 step 10); "
                "model=%d dtype=%d N=%d", c->model, c->dtype, c->N);
  return set_detection(c, on, eps, (size_t)(7 * c->N - 3), false);
}

int vc_get_farkas(vc_ctx* c, int B, void* y, int flags) {
  return get_detection(c, "vc_get_farkas", VC_MODEL_KINEMATIC, B, y, nullptr, false, flags);
}

int vc_set_sqp_infeasibility(vc_ctx* c, int on, double eps) {
  if (!c) return VC_E_ARG;
  if (c->model != VC_MODEL_DYNAMIC || c->dtype != VC_F64 || !vc::st_sqp_built(c->N))
    return fail(c, VC_E_UNSUPPORTED,
                "vc_set_sqp_infeasibility: the single-track fp64 SQP kernel only (dynamic fp64, N=20..60 step 10); "
                "model=%d dtype=%d N=%d", c->model, c->dtype, c->N);
  if (!(c->p.dyn_mpc.trust_Fx > 0))
    return fail(c, VC_E_ARG, "vc_set_sqp_infeasibility: dyn_mpc.trust_Fx must be > 0 (it bounds |dz|_1)");
  return set_detection(c, on, eps, (size_t)(12 * c->N - 3), true);
}

int vc_get_sqp_farkas(vc_ctx* c, int B, void* y, int32_t* qp_index, int flags) {
  return get_detection(c, "vc_get_sqp_farkas", VC_MODEL_DYNAMIC, B, y, qp_index, true, flags);
}

int vc_set_sqp_regularization(vc_ctx* c, int levels, double factor) {
  if (!c) return VC_E_ARG;
  if (c->model != VC_MODEL_DYNAMIC || c->dtype != VC_F64 || !vc::st_sqp_built(c->N))
    return fail(c, VC_E_UNSUPPORTED,
                "vc_set_sqp_regularization: the single-track fp64 SQP kernel only (dynamic fp64, N=20..60 step 10); "
                "model=%d dtype=%d N=%d", c->model, c->dtype, c->N);
  if (levels < 0 || levels > 6) return fail(c, VC_E_ARG, "vc_set_sqp_regularization: levels=%d outside [0,6]", levels);
  const double f = factor <= 0.0 ? 10.0 : factor;  // (a NaN factor fails the test below)
  if (!(f > 1.0)) return fail(c, VC_E_ARG, "vc_set_sqp_regularization: factor=%g must be > 1 (<= 0 keeps 10)", factor);
  c->reg.levels = levels;
  c->reg.factor = f;
  c->reg.B = 0;  // no solve has written levels under this setting yet
  return 0;
}

int vc_get_sqp_regularization(vc_ctx* c, int B, int32_t* level, int flags) {
  if (int r = check_common(c, B, flags)) return r;
  const Regularize& g = c->reg;
  if (g.levels <= 0) return fail(c, VC_E_ARG, "vc_get_sqp_regularization: the regularised retry is off");
  if (B > g.B) return fail(c, VC_E_ARG, "vc_get_sqp_regularization: B=%d exceeds the last solve's %d", B, g.B);
  if (!level) return fail(c, VC_E_ARG, "null pointer");
  if (B == 0) return 0;
  const hipMemcpyKind kind = flags == VC_DEVICE_PTRS ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  VC_HIP(c, hipMemcpyAsync(level, g.level, (size_t)B * g.K * 4, kind, c->stream));
  if (flags != VC_DEVICE_PTRS) VC_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

int vc_debug_sqp_breakdown(vc_ctx* c, int sqp_iter, int problem, int levels) {
  if (!c) return VC_E_ARG;
  c->reg.dbg_sqp_iter = sqp_iter;
  c->reg.dbg_problem = problem;
  c->reg.dbg_levels = levels;
  return 0;
}

int vc_set_casc_infeasibility(vc_ctx* c, int on, double eps) {
  if (!c) return VC_E_ARG;
  if (c->model != VC_MODEL_CASCADED || c->dtype != VC_F64 || !vc::casc_ric_built(c->N, c->p.casc.horizon_pm))
    return fail(c, VC_E_UNSUPPORTED,
                "vc_set_casc_infeasibility: the stagewise cascaded fp64 SQP kernel only (cascaded fp64, N=20, "
                "horizon_pm=15/25/35/40); model=%d dtype=%d N=%d horizon_pm=%d", c->model, c->dtype, c->N,
                c->p.casc.horizon_pm);
  if (c->p.qp.solver == 2)
    return fail(c, VC_E_UNSUPPORTED,
                "vc_set_casc_infeasibility: qp.solver=2 asks for the condensed kernel, which has no detection");
  if (!(c->p.dyn_mpc.trust_Fx > 0))
    return fail(c, VC_E_ARG, "vc_set_casc_infeasibility: dyn_mpc.trust_Fx must be > 0 (it bounds |dz|_1)");
  // rows in oracle/casc_sqp.py casc_qp's order: 12N - 3 single-track, 6 per point-mass stage
  return set_detection(c, on, eps, (size_t)(12 * c->N - 3 + 6 * c->p.casc.horizon_pm), true);
}

int vc_get_casc_farkas(vc_ctx* c, int B, void* y, int32_t* qp_index, int flags) {
  return get_detection(c, "vc_get_casc_farkas", VC_MODEL_CASCADED, B, y, qp_index, true, flags);
}

static int kin_solve(vc_ctx* c, int B, const void* x0, const void* kappa, const void* ds, void* xbar,
                     const void* ubar_in, void* u_out, void* u0, int32_t* status, int32_t* iters, void* diag,
                     int flags);

int vc_solve(vc_ctx* c, int B, const void* x0, const void* kappa, const void* ds, void* xbar, void* ubar, void* u0,
             int32_t* status, int32_t* iters, int flags) {
  return vc_solve_diag(c, B, x0, kappa, ds, xbar, ubar, u0, status, iters, nullptr, flags);
}

int vc_solve_from(vc_ctx* c, int B, const void* x0, const void* kappa, const void* ds, const void* ubar_in,
                  void* xbar, void* u_out, void* u0, int32_t* status, int32_t* iters, int flags) {
  if (int r = check_common(c, B, flags)) return r;
  if (!ubar_in || !u_out) return fail(c, VC_E_ARG, "null pointer");
  if (ubar_in == u_out) return vc_solve(c, B, x0, kappa, ds, xbar, u_out, u0, status, iters, flags);
  if (c->model == VC_MODEL_KINEMATIC && kin_solve_built(c)) {
    if (!x0 || !kappa || !ds || !xbar || !u0 || !status || !iters) return fail(c, VC_E_ARG, "null pointer");
    if (B == 0) return 0;
    return kin_solve(c, B, x0, kappa, ds, xbar, ubar_in, u_out, u0, status, iters, nullptr, flags);
  }
  // the SQP contexts iterate in place: u_out <- ubar_in, then vc_solve on u_out
  const int H = c->N + (c->model == VC_MODEL_CASCADED ? c->p.casc.horizon_pm : 0);
  const size_t bytes = (size_t)B * H * 2 * (c->dtype == VC_F32 ? 4 : 8);
  if (flags == VC_HOST_PTRS) std::memcpy(u_out, ubar_in, bytes);
  else VC_HIP(c, hipMemcpyAsync(u_out, ubar_in, bytes, hipMemcpyDeviceToDevice, c->stream));
  return vc_solve(c, B, x0, kappa, ds, xbar, u_out, u0, status, iters, flags);
}

int vc_solve_diag(vc_ctx* c, int B, const void* x0, const void* kappa, const void* ds, void* xbar, void* ubar,
                  void* u0, int32_t* status, int32_t* iters, void* diag, int flags) {
  if (int r = check_common(c, B, flags)) return r;
  if (!kin_solve_built(c) && !dyn_solve_built(c) && !casc_solve_built(c))
    return fail(c, VC_E_UNSUPPORTED,
                "vc_solve: model=%d dtype=%d N=%d not built (kinematic fp64 N=10..60 step 10, dynamic fp64 "
                "N=20..60 step 10, dynamic fp32 N=40, cascaded fp64 N=20 + 40 are)", c->model, c->dtype, c->N);
  if (!x0 || !kappa || !ds || !xbar || !ubar || !u0 || !status || !iters) return fail(c, VC_E_ARG, "null pointer");
  if (B == 0) return 0;
  if (c->model == VC_MODEL_DYNAMIC) return dyn_solve(c, B, x0, kappa, ds, xbar, ubar, u0, status, iters, diag, flags);
  if (c->model == VC_MODEL_CASCADED) return casc_solve(c, B, x0, kappa, ds, xbar, ubar, u0, status, iters, diag, flags);
  return kin_solve(c, B, x0, kappa, ds, xbar, ubar, ubar, u0, status, iters, diag, flags);
}

// The kinematic solve with the warm start read through ubar_in and u* written through u_out
// (vc_solve: both the caller's ubar; vc_solve_from: two buffers).
static int kin_solve(vc_ctx* c, int B, const void* x0, const void* kappa, const void* ds, void* xbar,
                     const void* ubar_in, void* u_out, void* u0, int32_t* status, int32_t* iters, void* diag,
                     int flags) {
  if (c->p.qp.elastic < 0.0 && c->p.qp.kin_sqp <= 0)
    return fail(c, VC_E_ARG, "vc_qp.elastic < 0 (elastic on failure) needs kin_sqp > 0; rho > 0 for one QP step");
  const int N = c->N, nx = 6, nu = 2;
  vc::KinLtvArgs a{};
  a.mode = 0;
  a.B = B;
  a.L = c->p.kin_car.l;
  a.w = c->p.kin_mpc;
  a.qp = c->p.qp;
  a.obs = c->p.obs;
  const size_t u_bytes = (size_t)B * N * nu * 8, x_bytes = (size_t)B * (N + 1) * nx * 8;
  Staging st(c, flags);
  if (int r = st.bind([&] {
        a.x0 = st.in(x0, (size_t)B * nx * 8);
        a.kappa = st.in(kappa, (size_t)B * N * 8);
        a.ds = st.in(ds, (size_t)B * N * 8);
        // the warm start comes from ubar_in and u* goes back through u_out: one slice, two host pointers
        const Staging::Pair u = st.pair(ubar_in, u_out, u_bytes);
        a.ubar = u.rd;
        a.u_out = u.wr;
        // multiple shooting (qp.ms): the warm-start states arrive in xbar
        a.x_in = a.x_out = st.pair(c->p.qp.ms ? xbar : nullptr, xbar, x_bytes).wr;
        a.u0 = st.out(u0, (size_t)B * nu * 8);
        a.status = st.out(status, (size_t)B * 4);
        a.iters = st.out(iters, (size_t)B * 4);
        a.diag = st.out(diag, (size_t)B * VC_DIAG_COLS * 8);
      }))
    return r;
  // detection on: the launches below are the stagewise kernel's DET instantiation, or, where a
  // qp.solver = 2 context keeps the condensed kernel (kin_condensed), kin_ltv_kernel<N, true>
  arm_detection(c, a, B);
  const int S = c->p.qp.kin_sqp;
  if (S > 0 && (const void*)a.ubar != (const void*)a.u_out) {
    // the SQP iterates in place: start it on u_out (device pointers; staged, the two are one slice)
    VC_HIP(c, hipMemcpyAsync(a.u_out, a.ubar, u_bytes, hipMemcpyDeviceToDevice, c->stream));
    a.ubar = a.u_out;
  }
  if (S <= 0) {  // the LTV-QP contract: one QP step
    if (kin_condensed(c)) VC_HIP(c, vc::launch_kin_ltv(a, N, c->stream));
    else VC_HIP(c, vc::launch_kin_ric(a, N, c->stream));
  } else {
    // globalised step (oracle/kin_sqp.py): S x { QP step at ubar; merit line search }
    const size_t o_up = 0, o_st = al256(u_bytes), o_it = o_st + al256((size_t)B * 4),
                 o_xp = o_it + al256((size_t)B * 4), total = o_xp + al256(x_bytes);
    if (int r = ensure_scratch(c, &c->ls, &c->ls_bytes, total)) return r;
    char* base = static_cast<char*>(c->ls);
    vc::KinMeritArgs m{};
    m.x0 = a.x0;
    m.kappa = a.kappa;
    m.ds = a.ds;
    m.u_prev = (const double*)(base + o_up);
    m.ubar = a.u_out;
    m.x_out = a.x_out;
    m.u0 = a.u0;
    m.qp_status = a.status;
    m.qp_iters = a.iters;
    m.status = a.status;
    m.iters = a.iters;
    m.st_acc = (int32_t*)(base + o_st);
    m.it_acc = (int32_t*)(base + o_it);
    m.ls_diag = nullptr;
    m.ms = c->p.qp.ms;
    m.restart = S > 1;
    m.x_prev = (const double*)(base + o_xp);
    m.B = B;
    m.N = N;
    m.L = a.L;
    m.w = a.w;
    m.obs = a.obs;
    // qp.elastic < 0: hard rows first, elastic rows only where those fail (stagewise kernel only)
    const bool elastic_retry = c->p.qp.elastic < 0.0 && !kin_condensed(c);
    if (c->p.qp.elastic < 0.0) a.qp.elastic = 0.0;
    for (int i = 0; i < S; ++i) {
      VC_HIP(c, hipMemcpyAsync(base + o_up, a.u_out, u_bytes, hipMemcpyDeviceToDevice, c->stream));
      if (m.ms) VC_HIP(c, hipMemcpyAsync(base + o_xp, a.x_out, x_bytes, hipMemcpyDeviceToDevice, c->stream));
      if (kin_condensed(c)) VC_HIP(c, vc::launch_kin_ltv(a, N, c->stream));
      else VC_HIP(c, vc::launch_kin_ric(a, N, c->stream));
      if (elastic_retry) {
        // elastic on failure: the QPs the hard-row pass left non-solved, again from the same
        // iterate (the pre-step copies: the first pass has overwritten ubar / xbar in place)
        vc::KinLtvArgs e = a;
        e.qp.elastic = c->p.qp.elastic;
        e.ubar = (const double*)(base + o_up);
        if (m.ms) e.x_in = (const double*)(base + o_xp);
        VC_HIP(c, vc::launch_kin_ric(e, N, c->stream));
      }
      if (i == c->fault_iter && c->fault_problem >= 0 && c->fault_problem < B)
        VC_HIP(c, vc::launch_kin_qp_fault(a, N, c->fault_problem, c->stream));
      m.first = i == 0;
      VC_HIP(c, vc::launch_kin_merit(m, c->stream));
    }
  }
  return st.finish();
}

int vc_solve_debug(vc_ctx* c, int B, const void* x0, const void* kappa, const void* ds, void* xbar, void* ubar,
                   void* u0, int32_t* status, int32_t* iters, void* dbg, int flags) {
  if (int r = check_common(c, B, flags)) return r;
  if (!dyn_solve_built(c)) return fail(c, VC_E_UNSUPPORTED, "vc_solve_debug: dynamic fp32 N=40 contexts only");
  if (!x0 || !kappa || !ds || !xbar || !ubar || !u0 || !status || !iters || !dbg)
    return fail(c, VC_E_ARG, "null pointer");
  if (B == 0) return 0;
  return dyn_solve(c, B, x0, kappa, ds, xbar, ubar, u0, status, iters, nullptr, flags, dbg);
}

int vc_debug_stride(void) { return vc::dyn_sqp_debug_stride(); }

int vc_debug_rcp(vc_ctx* c, int n, const void* x, void* out, int flags) {
  if (!c) return VC_E_ARG;
  if (n < 0 || n > c->max_batch) return fail(c, VC_E_ARG, "n %d outside [0, max_batch=%d]", n, c->max_batch);
  if (int r = check_common(c, 0, flags)) return r;
  if (!x || !out) return fail(c, VC_E_ARG, "null pointer");
  if (n == 0) return 0;
  Ptr dx, dout;
  Staging st(c, flags);
  if (int r = st.bind([&] {
        dx = st.in(x, (size_t)n * 8);
        dout = st.out(out, (size_t)n * 32);
      }))
    return r;
  VC_HIP(c, vc::launch_rcp_probe(n, dx, dout, c->stream));
  return st.finish();
}

int vc_debug_kin_gdots(vc_ctx* c, int B, const void* G, const void* vz, const void* vc, void* out_grow,
                       void* out_gt, int flags) {
  if (int r = check_common(c, B, flags)) return r;
  if (c->model != VC_MODEL_KINEMATIC || c->dtype != VC_F64 || vc::kin_ltv_smem_bytes(c->N) == 0)
    return fail(c, VC_E_UNSUPPORTED, "vc_debug_kin_gdots: kinematic fp64 contexts with the fused kernel's N only");
  if (!G || !vz || !vc || !out_grow || !out_gt) return fail(c, VC_E_ARG, "null pointer");
  if (B == 0) return 0;
  const int N = c->N, n = 2 * N, NC = 2 * (N - 1);
  Ptr dG, dvz, dvc, dgrow, dgt;
  Staging st(c, flags);
  if (int r = st.bind([&] {
        dG = st.in(G, (size_t)B * NC * n * 8);
        dvz = st.in(vz, (size_t)B * n * 8);
        dvc = st.in(vc, (size_t)B * NC * 8);
        dgrow = st.out(out_grow, (size_t)B * 64 * 8);
        dgt = st.out(out_gt, (size_t)B * 64 * 8);
      }))
    return r;
  VC_HIP(c, vc::launch_kin_gdots(B, N, dG, dvz, dvc, dgrow, dgt, c->stream));
  return st.finish();
}

int vc_debug_kin_trisolve(vc_ctx* c, int B, const void* L, const void* dinv, const void* b, void* out, int flags) {
  if (int r = check_common(c, B, flags)) return r;
  if (c->model != VC_MODEL_KINEMATIC || c->dtype != VC_F64 || vc::kin_ltv_smem_bytes(c->N) == 0)
    return fail(c, VC_E_UNSUPPORTED, "vc_debug_kin_trisolve: kinematic fp64 contexts with the fused kernel's N only");
  if (!L || !dinv || !b || !out) return fail(c, VC_E_ARG, "null pointer");
  if (B == 0) return 0;
  const int N = c->N, n = 2 * N;
  Ptr dL, dd, db, dout;
  Staging st(c, flags);
  if (int r = st.bind([&] {
        dL = st.in(L, (size_t)B * n * n * 8);
        dd = st.in(dinv, (size_t)B * n * 8);
        db = st.in(b, (size_t)B * 64 * 8);
        dout = st.out(out, (size_t)B * 64 * 8);
      }))
    return r;
  VC_HIP(c, vc::launch_kin_trisolve(B, N, dL, dd, db, dout, c->stream));
  return st.finish();
}

int vc_debug_qp_fault(vc_ctx* c, int sqp_iter, int problem) {
  if (!c) return VC_E_ARG;
  c->fault_iter = sqp_iter;
  c->fault_problem = problem;
  return 0;
}

int vc_debug_kin_merit(vc_ctx* c, int B, const void* x0, const void* kappa, const void* ds, const void* u_prev,
                       void* u, const void* x_prev, void* x, int32_t* status, int32_t* iters, int32_t* st_acc,
                       int32_t* it_acc, int first, int restart, void* u0, void* ls_diag, int flags) {
  if (int r = check_common(c, B, flags)) return r;
  if (c->model != VC_MODEL_KINEMATIC || c->dtype != VC_F64)
    return fail(c, VC_E_UNSUPPORTED, "vc_debug_kin_merit: kinematic fp64 contexts only; model=%d dtype=%d", c->model,
                c->dtype);
  const bool ms = c->p.qp.ms != 0;
  if (!x0 || !kappa || !ds || !u_prev || !u || !x || !status || !iters || !st_acc || !it_acc || !u0 || !ls_diag ||
      (ms && !x_prev))
    return fail(c, VC_E_ARG, "null pointer");
  if (B == 0) return 0;
  const int N = c->N, nx = 6, nu = 2;
  const size_t u_bytes = (size_t)B * N * nu * 8, x_bytes = (size_t)B * (N + 1) * nx * 8;
  vc::KinMeritArgs m{};
  m.B = B;
  m.N = N;
  m.first = first != 0;
  m.restart = restart != 0;
  m.ms = ms;
  m.L = c->p.kin_car.l;
  m.w = c->p.kin_mpc;
  m.obs = c->p.obs;
  Staging st(c, flags);
  if (int r = st.bind([&] {
        m.x0 = st.in(x0, (size_t)B * nx * 8);
        m.kappa = st.in(kappa, (size_t)B * N * 8);
        m.ds = st.in(ds, (size_t)B * N * 8);
        m.u_prev = st.in(u_prev, u_bytes);
        m.ubar = st.inout(u, u_bytes);
        // the state iterate is read under multiple shooting only (kin_solve alike); x_prev is then
        // never dereferenced and stands on a valid buffer
        m.x_out = st.pair(ms ? x : nullptr, x, x_bytes).wr;
        m.x_prev = ms ? (const double*)st.in(x_prev, x_bytes) : (const double*)m.x_out;
        // the QP's status / iteration count in, the step's out: one buffer each, as kin_solve aliases them
        m.qp_status = m.status = st.inout(status, (size_t)B * 4);
        m.qp_iters = m.iters = st.inout(iters, (size_t)B * 4);
        m.st_acc = st.inout(st_acc, (size_t)B * 4);
        m.it_acc = st.inout(it_acc, (size_t)B * 4);
        m.u0 = st.out(u0, (size_t)B * nu * 8);
        m.ls_diag = st.out(ls_diag, (size_t)B * 4 * 8);
      }))
    return r;
  VC_HIP(c, vc::launch_kin_merit(m, c->stream));
  return st.finish();
}

int vc_condense(vc_ctx* c, int B, const void* x0, const void* ubar, const void* kappa, const void* ds, void* H,
                void* g, int flags) {
  if (int r = check_common(c, B, flags)) return r;
  const bool casc_cond = c->model == VC_MODEL_CASCADED && c->dtype == VC_F64 &&
                         vc::casc_sqp_built(c->N, c->p.casc.horizon_pm);
  if (!(kin_solve_built(c) && kin_condensed_cfg(c)) && !casc_cond)
    return fail(c, VC_E_UNSUPPORTED, "vc_condense: model=%d dtype=%d N=%d not built", c->model, c->dtype, c->N);
  if (!x0 || !kappa || !ds || !ubar || !H || !g) return fail(c, VC_E_ARG, "null pointer");
  if (B == 0) return 0;
  if (c->model == VC_MODEL_CASCADED)
    return casc_solve(c, B, x0, kappa, ds, nullptr, const_cast<void*>(ubar), nullptr, nullptr, nullptr, nullptr, flags,
                      1, H, g);
  const int N = c->N, n = 2 * N;
  vc::KinLtvArgs a{};
  a.mode = 1;
  a.B = B;
  a.L = c->p.kin_car.l;
  a.w = c->p.kin_mpc;
  a.qp = c->p.qp;
  a.obs = c->p.obs;
  Staging st(c, flags);
  if (int r = st.bind([&] {
        a.x0 = st.in(x0, (size_t)B * 6 * 8);
        a.kappa = st.in(kappa, (size_t)B * N * 8);
        a.ds = st.in(ds, (size_t)B * N * 8);
        a.ubar = st.in(ubar, (size_t)B * n * 8);
        a.H_out = st.out(H, (size_t)B * n * n * 8);
        a.g_out = st.out(g, (size_t)B * n * 8);
      }))
    return r;
  VC_HIP(c, vc::launch_kin_ltv(a, N, c->stream));
  return st.finish();
}

int vc_rollout(vc_ctx* c, int B, const void* x0, const void* ubar, const void* kappa, const void* ds, void* xbar,
               int flags) {
  if (int r = check_common(c, B, flags)) return r;
  if (!x0 || !ubar || !kappa || !ds || !xbar) return fail(c, VC_E_ARG, "null pointer");
  if (B == 0) return 0;
  const int N = c->N, nx = nx_of(c);
  const size_t es = esize(c);
  vc::ModelArgs m = model_args(c, B);
  Ptr dx0, dubar, dkappa, dds, dxbar;
  Staging st(c, flags);
  if (int r = st.bind([&] {
        dx0 = st.in(x0, (size_t)B * nx * es);
        dubar = st.in(ubar, (size_t)B * N * 2 * es);
        dkappa = st.in(kappa, (size_t)B * N * es);
        dds = st.in(ds, (size_t)B * N * es);
        dxbar = st.out(xbar, (size_t)B * (N + 1) * nx * es);
      }))
    return r;
  VC_HIP(c, vc::launch_rollout(m, c->dtype, dx0, dubar, dkappa, dds, dxbar, c->stream));
  return st.finish();
}

int vc_linearize(vc_ctx* c, int B, const void* xbar, const void* ubar, const void* kappa, const void* ds, void* A,
                 void* Bm, int flags) {
  if (int r = check_common(c, B, flags)) return r;
  if (c->model != VC_MODEL_KINEMATIC || c->dtype != VC_F64)
    return fail(c, VC_E_UNSUPPORTED, "vc_linearize: only the kinematic fp64 model is built");
  if (!xbar || !ubar || !kappa || !ds || !A || !Bm) return fail(c, VC_E_ARG, "null pointer");
  if (B == 0) return 0;
  const int N = c->N;
  vc::ModelArgs m = model_args(c, B);
  Ptr dxbar, dubar, dkappa, dds, dA, dBm;
  Staging st(c, flags);
  if (int r = st.bind([&] {
        dxbar = st.in(xbar, (size_t)B * (N + 1) * 6 * 8);
        dubar = st.in(ubar, (size_t)B * N * 2 * 8);
        dkappa = st.in(kappa, (size_t)B * N * 8);
        dds = st.in(ds, (size_t)B * N * 8);
        dA = st.out(A, (size_t)B * N * 36 * 8);
        dBm = st.out(Bm, (size_t)B * N * 12 * 8);
      }))
    return r;
  VC_HIP(c, vc::launch_kin_linearize(m, dxbar, dubar, dkappa, dds, dA, dBm, c->stream));
  return st.finish();
}

int vc_plant_step(vc_ctx* c, int B, const void* x, const void* u, const void* kappa, double dt, void* x_next,
                  int flags) {
  if (int r = check_common(c, B, flags)) return r;
  if (!x || !u || !kappa || !x_next) return fail(c, VC_E_ARG, "null pointer");
  if (B == 0) return 0;
  const int nx = nx_of(c);
  const size_t es = esize(c);
  vc::ModelArgs m = model_args(c, B);
  Ptr dx, du, dkappa, dnext;
  Staging st(c, flags);
  if (int r = st.bind([&] {
        dx = st.in(x, (size_t)B * nx * es);
        du = st.in(u, (size_t)B * 2 * es);
        dkappa = st.in(kappa, (size_t)B * es);
        dnext = st.out(x_next, (size_t)B * nx * es);
      }))
    return r;
  VC_HIP(c, vc::launch_plant_step(m, c->dtype, dx, du, dkappa, dt, dnext, c->stream));
  return st.finish();
}

int vc_ode(vc_ctx* c, int B, const void* x, const void* u, const void* kappa, int space, void* f, int flags) {
  if (int r = check_common(c, B, flags)) return r;
  if (!x || !u || !kappa || !f) return fail(c, VC_E_ARG, "null pointer");
  if (space != 0 && space != 1) return fail(c, VC_E_ARG, "vc_ode: space must be 0 (temporal) or 1 (spatial)");
  if (B == 0) return 0;
  const int nx = nx_of(c);
  const size_t es = esize(c);
  vc::ModelArgs m = model_args(c, B);
  Ptr dx, du, dkappa, df;
  Staging st(c, flags);
  if (int r = st.bind([&] {
        dx = st.in(x, (size_t)B * nx * es);
        du = st.in(u, (size_t)B * 2 * es);
        dkappa = st.in(kappa, (size_t)B * es);
        df = st.out(f, (size_t)B * nx * es);
      }))
    return r;
  VC_HIP(c, vc::launch_ode(m, c->dtype, dx, du, dkappa, space, df, c->stream));
  return st.finish();
}

int vc_spatial_step(vc_ctx* c, int B, const void* x, const void* u, const void* kappa, const void* ds, void* x_next,
                    int flags) {
  if (int r = check_common(c, B, flags)) return r;
  if (!x || !u || !kappa || !ds || !x_next) return fail(c, VC_E_ARG, "null pointer");
  if (B == 0) return 0;
  const int nx = nx_of(c);
  const size_t es = esize(c);
  vc::ModelArgs m = model_args(c, B);
  Ptr dx, du, dkappa, dds, dnext;
  Staging st(c, flags);
  if (int r = st.bind([&] {
        dx = st.in(x, (size_t)B * nx * es);
        du = st.in(u, (size_t)B * 2 * es);
        dkappa = st.in(kappa, (size_t)B * es);
        dds = st.in(ds, (size_t)B * es);
        dnext = st.out(x_next, (size_t)B * nx * es);
      }))
    return r;
  VC_HIP(c, vc::launch_spatial_step(m, c->dtype, dx, du, dkappa, dds, dnext, c->stream));
  return st.finish();
}

int vc_track_set(vc_ctx* c, int n_pieces, double h, double length, const double* coef) {
  if (!c) return VC_E_ARG;
  if (n_pieces < 1 || !(h > 0) || !(length > 0) || !coef)
    return fail(c, VC_E_ARG, "vc_track_set: need n_pieces >= 1, h > 0, length > 0, coef");
  for (int i = 0; i < 4 * n_pieces; ++i)
    if (!std::isfinite(coef[i])) return fail(c, VC_E_ARG, "vc_track_set: coef[%d] not finite", i);
  VC_HIP(c, hipSetDevice(c->device));
  VC_HIP(c, hipStreamSynchronize(c->stream));  // no kernel may still read the old table
  if (c->track) VC_HIP(c, hipFree(c->track));
  c->track = nullptr;
  c->track_n = 0;
  VC_HIP(c, hipMalloc(&c->track, (size_t)n_pieces * 4 * sizeof(double)));
  VC_HIP(c, hipMemcpy(c->track, coef, (size_t)n_pieces * 4 * sizeof(double), hipMemcpyHostToDevice));
  c->track_n = n_pieces;
  c->track_h = h;
  c->track_len = length;
  return 0;
}

int vc_track_k(vc_ctx* c, int B, const void* s, void* k, int flags) {
  if (int r = check_common(c, B, flags)) return r;
  if (!s || !k) return fail(c, VC_E_ARG, "null pointer");
  if (!c->track) return fail(c, VC_E_ARG, "vc_track_k: no track table (vc_track_set)");
  if (B == 0) return 0;
  const size_t es = esize(c);
  Ptr dpos, dk;
  Staging st(c, flags);
  if (int r = st.bind([&] {
        dpos = st.in(s, B * es);
        dk = st.out(k, B * es);
      }))
    return r;
  VC_HIP(c, vc::launch_track_k(track_table(c), c->dtype, B, dpos, dk, c->stream));
  return st.finish();
}

int vc_horizon(vc_ctx* c, int B, const void* x0, const void* xbar, double mpc_dt, void* kappa, void* ds,
               int flags) {
  if (int r = check_common(c, B, flags)) return r;
  if (!x0 || !xbar || !kappa || !ds) return fail(c, VC_E_ARG, "null pointer");
  if (!c->track) return fail(c, VC_E_ARG, "vc_horizon: no track table (vc_track_set)");
  if (B == 0) return 0;
  const int N = c->N, nx = nx_of(c), NS = ns_of(c), NH = nh_of(c), M = NH - N;
  const double ds_pm = c->p.casc.ds_pm;
  const size_t es = esize(c);
  Ptr dx0, dxbar, dkappa, dds;
  Staging st(c, flags);
  if (int r = st.bind([&] {
        dx0 = st.in(x0, (size_t)B * nx * es);
        dxbar = st.in(xbar, (size_t)B * NS * nx * es);
        dkappa = st.out(kappa, (size_t)B * NH * es);
        dds = st.out(ds, (size_t)B * NH * es);
      }))
    return r;
  VC_HIP(c, vc::launch_horizon(track_table(c), c->model, c->dtype, B, N, M, ds_pm, dx0, c->dtype == VC_F64, dxbar,
                               mpc_dt, dkappa, dds, nullptr, c->stream));
  return st.finish();
}

int vc_drive(vc_ctx* c, int B, double* x64, const void* u0, double dt, void* x_ctx, int flags) {
  if (int r = check_common(c, B, flags)) return r;
  if (!x64 || !u0) return fail(c, VC_E_ARG, "null pointer");
  if (!c->track) return fail(c, VC_E_ARG, "vc_drive: no track table (vc_track_set)");
  if (B == 0) return 0;
  const int nx = nx_of(c);
  const size_t es = esize(c);
  vc::ModelArgs m = model_args(c, B);
  Ptr dx, du0, dctx;
  Staging st(c, flags);
  if (int r = st.bind([&] {
        dx = st.inout(x64, (size_t)B * nx * 8);
        du0 = st.in(u0, (size_t)B * 2 * es);
        dctx = st.out(x_ctx, (size_t)B * nx * es);
      }))
    return r;
  VC_HIP(c, vc::launch_drive(m, c->dtype, track_table(c), dx, du0, dt, dctx, nullptr, nullptr, nullptr, nullptr,
                             nullptr, nullptr, nullptr, c->stream));
  return st.finish();
}

int vc_simulate(vc_ctx* c, int B, int steps, double mpc_dt, double dt, double* x64, void* xbar, void* ubar,
                double* log_x, void* log_u, int32_t* nfail, int flags) {
  if (int r = check_common(c, B, flags)) return r;
  if (!x64 || !xbar || !ubar) return fail(c, VC_E_ARG, "null pointer");
  if (steps < 0) return fail(c, VC_E_ARG, "steps %d < 0", steps);
  if (!c->track) return fail(c, VC_E_ARG, "vc_simulate: no track table (vc_track_set)");
  if (!kin_solve_built(c) && !dyn_solve_built(c) && !casc_solve_built(c))
    return fail(c, VC_E_UNSUPPORTED, "vc_simulate: model=%d dtype=%d N=%d has no built vc_solve", c->model, c->dtype,
                c->N);
  if (B == 0 || steps == 0) return 0;
  const int N = c->N, nx = nx_of(c), NS = ns_of(c), NH = nh_of(c), M = NH - N;
  const double ds_pm = c->p.casc.ds_pm;
  const size_t es = esize(c), x_bytes = (size_t)B * nx * 8;
  double *dx, *dlx;
  void *dxbar, *dubar, *dlu;
  int32_t* dnf;
  Staging st(c, flags);
  if (int r = st.bind([&] {
        dx = st.inout(x64, x_bytes);
        dxbar = st.inout(xbar, (size_t)B * NS * nx * es);
        dubar = st.inout(ubar, (size_t)B * NH * 2 * es);
        dlx = st.out(log_x, (size_t)(steps + 1) * B * nx * 8);
        dlu = st.out(log_u, (size_t)steps * B * 2 * es);
        dnf = st.inout(nfail, (size_t)B * 4);
      }))
    return r;
  // scratch: kappa[B][NH], ds[B][NH], x[B][nx], u0[B][2] (context dtype), status[B], iters[B]
  const size_t o_kap = 0, o_ds = o_kap + al256((size_t)B * NH * es), o_x = o_ds + al256((size_t)B * NH * es),
               o_u0 = o_x + al256((size_t)B * nx * es), o_st = o_u0 + al256((size_t)B * 2 * es),
               o_it = o_st + al256((size_t)B * 4), total = o_it + al256((size_t)B * 4);
  if (int r = ensure_scratch(c, &c->sim, &c->sim_bytes, total)) return r;
  char* base = static_cast<char*>(c->sim);
  void *kap = base + o_kap, *dsv = base + o_ds, *xc = base + o_x, *u0 = base + o_u0;
  int32_t *stat = (int32_t*)(base + o_st), *it = (int32_t*)(base + o_it);
  const vc::TrackTable tt = track_table(c);
  vc::ModelArgs m = model_args(c, B);
  if (dlx) VC_HIP(c, hipMemcpyAsync(dlx, dx, x_bytes, hipMemcpyDeviceToDevice, c->stream));
  for (int step = 0; step < steps; ++step) {
    VC_HIP(c, vc::launch_horizon(tt, c->model, c->dtype, B, N, M, ds_pm, dx, true, dxbar, mpc_dt, kap, dsv, xc,
                                 c->stream));
    if (int r = vc_solve_diag(c, B, xc, kap, dsv, dxbar, dubar, u0, stat, it, nullptr, VC_DEVICE_PTRS)) return r;
    VC_HIP(c, vc::launch_drive(m, c->dtype, tt, dx, u0, dt, nullptr, stat, dxbar, dubar, dnf,
                               dlx ? dlx + (size_t)(step + 1) * B * nx : nullptr,
                               dlu ? (char*)dlu + (size_t)step * B * 2 * es : nullptr, kap, c->stream));
  }
  return st.finish();
}

}  // extern "C"
