// os2r_sysid_capi.hip — the C-ABI of libos2r_sysid.so (include/os2r_sysid.h): the entry points' own argument checks and their
// launches; the check of the layout, the device guard, the gfx950 check and the calling thread's error text are os2r_host.hpp's.
// Every argument check runs before the first HIP call.
#include "os2r_sysid.hpp"

// two entry points, two prefixes: each names itself here on entry, and os2r_host.hpp's fail() puts that name in front
namespace {
thread_local const char* g_entry_point = "";
}
#define OS2R_HOST_ERROR_PREFIX g_entry_point
#include "os2r_host.hpp"

using namespace os2r;

namespace {

// one device array of a call: [at, at + bytes)
struct Span {
  const char* name;
  const void* at;
  uintptr_t bytes;
  bool output;
};

bool overlap(const Span& a, const Span& b) {
  const uintptr_t x = (uintptr_t)a.at, y = (uintptr_t)b.at;
  return x < y + b.bytes && y < x + a.bytes;
}

// every output against every input and every output before it -> the refusal's text, or an empty string
std::string overlap_refusal(const Span* spans, int count) {
  for (int o = 0; o < count; ++o)
    for (int i = 0; spans[o].output && spans[o].at && i < o; ++i)
      if (spans[i].at && overlap(spans[o], spans[i])) return std::string(spans[o].name) + " overlaps " + spans[i].name;
  return std::string();
}

// the first required array that is null -> "null <name>", or an empty string
std::string null_refusal(const Span* spans, int count, const char* const* optional, int noptional) {
  for (int i = 0; i < count; ++i) {
    bool may = false;
    for (int k = 0; k < noptional; ++k) may = may || std::strcmp(spans[i].name, optional[k]) == 0;
    if (!spans[i].at && !may) return std::string("null ") + spans[i].name;
  }
  return std::string();
}

// a * b * c bytes, held below 2^62 (the counts of a refused call may be anything)
uintptr_t bytes_of(uint64_t a, uint64_t b, uint64_t c) {
  const unsigned __int128 n = (unsigned __int128)a * b * c, top = (unsigned __int128)1 << 62;
  return (uintptr_t)(n > top ? top : n);
}

// the bits of a caller's double, read from memory (os2r_host.hpp says why)
__attribute__((noinline)) bool is_nan(const double* x) {
  uint64_t b;
  std::memcpy(&b, x, sizeof(b));
  return (b & 0x7fffffffffffffffull) > 0x7ff0000000000000ull;
}

// finite and > 0, as a double and rounded to float
__attribute__((noinline)) bool is_step(const double* x, bool as_float) {
  uint64_t b;
  std::memcpy(&b, x, sizeof(b));
  if ((b >> 63) != 0u || ((b >> 52) & 0x7ffu) == 0x7ffu || b == 0u) return false;
  if (!as_float) return true;
  volatile float f = (float)*x;
  const float g = f;
  uint32_t w;
  std::memcpy(&w, &g, sizeof(w));
  return ((w >> 23) & 0xffu) != 0xffu && w != 0u;
}

// what both entry points refuse about the counts, the steps and the bounds, as the refusal's text (null: nothing)
const char* shape_refusal(const Os2rControlLayout* layout, int32_t nparams, int64_t nsets, int64_t nsegments, const double* h_host,
                          const double* lo_host, const double* hi_host) {
  if (nparams < 1 || nparams > OS2RI_MAX_PARAMS) return "nparams must be 1..21";
  if (nsets < 1) return "nsets must be >= 1";
  if (nsets > OS2RI_MAX_SETS) return "nsets must be < 2^26 (a wave per set in one grid)";
  if (nsegments < 1) return "nsegments must be >= 1";
  if (nsegments % nsets != 0) return "nsegments must be a multiple of nsets";
  if (nsegments > 0x7fffffffll / (2 * nparams + 1)) return "(2 nparams + 1) * nsegments exceeds 2^31 - 1";
  if (!h_host) return "null h_host";
  if (!lo_host) return "null lo_host";
  if (!hi_host) return "null hi_host";
  for (int p = 0; p < nparams; ++p) {
    if (!is_step(&h_host[p], layout->dtype == OS2R_F32)) return "h_host entries must be finite and > 0 in the layout's dtype";
    if (is_nan(&lo_host[p]) || is_nan(&hi_host[p])) return "lo_host and hi_host entries must not be NaN";
    if (lo_host[p] > hi_host[p]) return "lo_host must be <= hi_host";
  }
  return nullptr;
}

// sel_host -> the rows of the packed parameters, or the refusal's text
const char* rows_refusal(const Os2rControlLayout* layout, int32_t nparams, const int32_t* sel_host, int* row) {
  if (!sel_host) return "null sel_host";
  for (int p = 0; p < nparams; ++p) {
    const int32_t field = sel_host[2 * p], entry = sel_host[2 * p + 1];
    if (field < OS2R_PARAM_MASS_SCALE || field > OS2R_PARAM_GRAVITY) return "sel_host fields must be 0..4";
    if (entry < 0 || entry >= (field == OS2R_PARAM_GRAVITY ? 1 : layout->nq)) return "sel_host entries must be 0..nq-1, 0 for gravity";
    row[p] = field * layout->nq + entry;
    for (int q = 0; q < p; ++q)
      if (row[q] == row[p]) return "sel_host names a parameter twice";
  }
  return nullptr;
}

// the first field of the constants that is not finite -> its name, or null
const char* constants_refusal(const Os2riConstants* k) {
  static const char* const names[] = {"shrink", "grow", "lam_min", "lam_max", "diag_floor", "tol", "cost_floor"};
  static_assert(sizeof(Os2riConstants) == sizeof(names) / sizeof(names[0]) * sizeof(double), "seven doubles");
  const double* const v = &k->shrink;
  for (unsigned i = 0; i < sizeof(names) / sizeof(names[0]); ++i)
    if (!is_finite(&v[i])) return names[i];
  return nullptr;
}

template <typename T>
void fill_steps(SysidArgs<T>& p, int32_t nparams, const double* h_host, const double* lo_host, const double* hi_host) {
  for (int i = 0; i < nparams; ++i) {
    p.h[i] = (T)h_host[i];
    p.lo[i] = (T)lo_host[i];
    p.hi[i] = (T)hi_host[i];
  }
}

}  // namespace

extern "C" {

int os2ri_abi_version(void) { return OS2R_SYSID_ABI_VERSION; }

const char* os2ri_last_error(void) { return g_error.c_str(); }

int os2ri_perturb(const Os2rControlLayout* layout, int32_t nparams, int64_t nsets, int64_t nsegments, const int32_t* sel_host,
                  const double* h_host, const double* lo_host, const double* hi_host, const void* theta_dev, const void* base_dev,
                  void* params_dev, void* stream) {
  g_entry_point = "os2ri_perturb: ";
  if (const char* why = layout_refusal(layout)) return fail(OS2R_ERR_INVALID, why);
  if (const char* why = shape_refusal(layout, nparams, nsets, nsegments, h_host, lo_host, hi_host)) return fail(OS2R_ERR_INVALID, why);
  int row[OS2RI_MAX_PARAMS] = {0};
  if (const char* why = rows_refusal(layout, nparams, sel_host, row)) return fail(OS2R_ERR_INVALID, why);
  const uintptr_t elem = layout->dtype == OS2R_F64 ? sizeof(double) : sizeof(float);
  const int F = 4 * layout->nq + 1;
  if ((uint64_t)F * (2 * (uint64_t)nparams + 1) * (uint64_t)nsegments > 0xffffffffull)
    return fail(OS2R_ERR_INVALID, "(4 nq + 1) * (2 nparams + 1) * nsegments exceeds 2^32 - 1 (a thread per entry of params_dev)");
  {
    const uint64_t P = (uint64_t)nparams, M = (uint64_t)nsegments, N = (2 * P + 1) * M;
    const Span spans[] = {
        {"theta_dev", theta_dev, bytes_of((uint64_t)nsets, P, elem), false},
        {"base_dev", base_dev, bytes_of((uint64_t)F, M, elem), false},
        {"params_dev", params_dev, bytes_of((uint64_t)F, N, elem), true},
    };
    const int count = sizeof(spans) / sizeof(spans[0]);
    std::string why = null_refusal(spans, count, nullptr, 0);
    if (!why.empty()) return fail(OS2R_ERR_INVALID, why);
    why = overlap_refusal(spans, count);
    if (!why.empty()) return fail(OS2R_ERR_INVALID, why);
  }
  // the device, from here on
  if (const int rc = check_device(layout->device)) return rc;
  DeviceGuard guard(layout->device);
  auto launch = [&](auto real) {
    using T = decltype(real);
    SysidArgs<T> p;
    std::memset(&p, 0, sizeof(p));
    p.theta = (const T*)theta_dev; p.base = (const T*)base_dev; p.params = (T*)params_dev;
    p.sets = nsets; p.M = nsegments; p.P = nparams; p.F = F;
    for (int i = 0; i < nparams; ++i) p.row[i] = row[i];
    fill_steps<T>(p, nparams, h_host, lo_host, hi_host);
    launch_sysid_perturb<T>(p, (hipStream_t)stream);
    return launched(0);
  };
  return layout->dtype == OS2R_F64 ? launch(double()) : launch(float());
}

int os2ri_update(const Os2rControlLayout* layout, int32_t nparams, int64_t nsets, int64_t nsegments, int32_t nsteps, const double* h_host,
                 const double* lo_host, const double* hi_host, const Os2riConstants* constants, const void* obs_dev, const void* meas_dev,
                 const uint8_t* done_dev, const void* prec_dev, const void* theta_dev, const void* theta_best_dev, const void* cost_best_dev,
                 const void* hess_dev, const void* grad_dev, const void* lam_dev, const int32_t* status_dev, const int32_t* iters_dev,
                 void* theta_best_out_dev, void* cost_best_out_dev, void* hess_out_dev, void* grad_out_dev, void* lam_out_dev,
                 int32_t* status_out_dev, int32_t* iters_out_dev, void* theta_next_dev, void* cost_dev, int32_t* valid_dev,
                 uint8_t* accepted_dev, int32_t* failed_dev, void* delta_dev, void* sums_dev, int32_t* counts_dev, void* stream) {
  g_entry_point = "os2ri_update: ";
  if (const char* why = layout_refusal(layout)) return fail(OS2R_ERR_INVALID, why);
  if (layout->obs_dim < 1 || layout->obs_dim > OS2R_MAX_OBS) return fail(OS2R_ERR_INVALID, "layout->obs_dim must be 1..12");
  if (const char* why = shape_refusal(layout, nparams, nsets, nsegments, h_host, lo_host, hi_host)) return fail(OS2R_ERR_INVALID, why);
  if (nsteps < 1) return fail(OS2R_ERR_INVALID, "nsteps must be >= 1");
  if (!constants) return fail(OS2R_ERR_INVALID, "null constants");
  if (const char* field = constants_refusal(constants)) return fail(OS2R_ERR_INVALID, std::string("constants->") + field + " must be finite");
  if (constants->lam_min < 0.0) return fail(OS2R_ERR_INVALID, "constants->lam_min must be >= 0");
  if (!(constants->diag_floor > 0.0)) return fail(OS2R_ERR_INVALID, "constants->diag_floor must be > 0");
  const uintptr_t elem = layout->dtype == OS2R_F64 ? sizeof(double) : sizeof(float);
  {
    const uint64_t P = (uint64_t)nparams, T = (uint64_t)nsets, M = (uint64_t)nsegments, N = (2 * P + 1) * M, K = (uint64_t)nsteps,
                   D = (uint64_t)layout->obs_dim, E = P * (P + 1) / 2 + P + 1, i32 = sizeof(int32_t);
    const Span spans[] = {
        {"obs_dev", obs_dev, bytes_of(K * D, N, elem), false},
        {"meas_dev", meas_dev, bytes_of(K * D, M, elem), false},
        {"done_dev", done_dev, bytes_of(K, N, 1), false},
        {"prec_dev", prec_dev, bytes_of(D, 1, elem), false},
        {"theta_dev", theta_dev, bytes_of(T, P, elem), false},
        {"theta_best_dev", theta_best_dev, bytes_of(T, P, elem), false},
        {"cost_best_dev", cost_best_dev, bytes_of(T, 1, elem), false},
        {"hess_dev", hess_dev, bytes_of(T, P * P, elem), false},
        {"grad_dev", grad_dev, bytes_of(T, P, elem), false},
        {"lam_dev", lam_dev, bytes_of(T, 1, elem), false},
        {"status_dev", status_dev, bytes_of(T, 1, i32), false},
        {"iters_dev", iters_dev, bytes_of(T, 1, i32), false},
        {"theta_best_out_dev", theta_best_out_dev, bytes_of(T, P, elem), true},
        {"cost_best_out_dev", cost_best_out_dev, bytes_of(T, 1, elem), true},
        {"hess_out_dev", hess_out_dev, bytes_of(T, P * P, elem), true},
        {"grad_out_dev", grad_out_dev, bytes_of(T, P, elem), true},
        {"lam_out_dev", lam_out_dev, bytes_of(T, 1, elem), true},
        {"status_out_dev", status_out_dev, bytes_of(T, 1, i32), true},
        {"iters_out_dev", iters_out_dev, bytes_of(T, 1, i32), true},
        {"theta_next_dev", theta_next_dev, bytes_of(T, P, elem), true},
        {"cost_dev", cost_dev, bytes_of(T, 1, elem), true},
        {"valid_dev", valid_dev, bytes_of(T, 1, i32), true},
        {"accepted_dev", accepted_dev, bytes_of(T, 1, 1), true},
        {"failed_dev", failed_dev, bytes_of(T, 1, i32), true},
        {"delta_dev", delta_dev, bytes_of(T, P, elem), true},
        {"sums_dev", sums_dev, bytes_of(E, M + T, elem), true},
        {"counts_dev", counts_dev, bytes_of(M + T, 1, i32), true},
    };
    const int count = sizeof(spans) / sizeof(spans[0]);
    static const char* const optional[] = {"done_dev", "cost_dev", "valid_dev", "accepted_dev", "failed_dev", "delta_dev"};
    std::string why = null_refusal(spans, count, optional, 6);
    if (!why.empty()) return fail(OS2R_ERR_INVALID, why);
    why = overlap_refusal(spans, count);
    if (!why.empty()) return fail(OS2R_ERR_INVALID, why);
  }
  // the device, from here on
  if (const int rc = check_device(layout->device)) return rc;
  DeviceGuard guard(layout->device);
  auto launch = [&](auto real) {
    using T = decltype(real);
    SysidArgs<T> p;
    std::memset(&p, 0, sizeof(p));
    p.obs = (const T*)obs_dev; p.meas = (const T*)meas_dev; p.done = done_dev; p.prec = (const T*)prec_dev; p.theta = (const T*)theta_dev;
    p.theta_best = (const T*)theta_best_dev; p.cost_best = (const T*)cost_best_dev; p.hess = (const T*)hess_dev; p.grad = (const T*)grad_dev;
    p.lam = (const T*)lam_dev; p.status = status_dev; p.iters = iters_dev;
    p.theta_best_out = (T*)theta_best_out_dev; p.cost_best_out = (T*)cost_best_out_dev; p.hess_out = (T*)hess_out_dev;
    p.grad_out = (T*)grad_out_dev; p.lam_out = (T*)lam_out_dev; p.status_out = status_out_dev; p.iters_out = iters_out_dev;
    p.theta_next = (T*)theta_next_dev; p.cost = (T*)cost_dev; p.valid = valid_dev; p.accepted = accepted_dev; p.failed = failed_dev;
    p.delta = (T*)delta_dev; p.sums = (T*)sums_dev; p.counts = counts_dev;
    p.sets = nsets; p.M = nsegments; p.P = nparams; p.K = nsteps; p.D = layout->obs_dim; p.F = 4 * layout->nq + 1;
    fill_steps<T>(p, nparams, h_host, lo_host, hi_host);
    const Os2riConstants& k = *constants;
    p.shrink = (T)k.shrink; p.grow = (T)k.grow; p.lam_min = (T)k.lam_min; p.lam_max = (T)k.lam_max; p.diag_floor = (T)k.diag_floor;
    p.tol = (T)k.tol; p.cost_floor = (T)k.cost_floor;
    launch_sysid_update<T>(p, (hipStream_t)stream);
    return launched(0);
  };
  return layout->dtype == OS2R_F64 ? launch(double()) : launch(float());
}

}  // extern "C"
