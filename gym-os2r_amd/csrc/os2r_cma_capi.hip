// os2r_cma_capi.hip — the C-ABI of libos2r_cma.so (include/os2r_cma.h): the entry points' own argument checks and their launches;
// the check of the layout, the device guard, the gfx950 check and the calling thread's error text are os2r_host.hpp's.
// Every argument check runs before the first HIP call.
#include "os2r_cma.hpp"

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

// what both entry points refuse about the populations' shape, as the refusal's text (null: nothing)
const char* shape_refusal(const Os2rControlLayout* layout, int64_t npops, int32_t nsamples, uint32_t flags) {
  if (layout->obs_dim < 1 || layout->obs_dim > OS2R_MAX_OBS) return "layout->obs_dim must be 1..12";
  if (npops < 1) return "npops must be >= 1";
  if (nsamples < 2) return "nsamples must be >= 2";
  if (nsamples > OS2RK_MAX_SAMPLES) return "nsamples must be < 2^27 (16 nsamples is a 32-bit counter word)";
  if (npops > 0x7fffffffll / nsamples) return "nsamples * npops exceeds 2^31 - 1";
  if (flags != 0u) return "unknown flag bits";
  return nullptr;
}

// the first field of the constants that is not finite -> its name, or null
const char* constants_refusal(const Os2rkCmaConstants* k) {
  static const char* const names[] = {"a_sigma", "b_sigma", "hsig_bound", "a_c", "b_c", "k0_moving", "k0_stalled",
                                      "c_1", "c_mu", "g_sigma", "chi", "sigma_min", "sigma_max"};
  static_assert(sizeof(Os2rkCmaConstants) == sizeof(names) / sizeof(names[0]) * sizeof(double), "thirteen doubles");
  const double* const v = &k->a_sigma;
  for (unsigned i = 0; i < sizeof(names) / sizeof(names[0]); ++i)
    if (!is_finite(&v[i])) return names[i];
  return nullptr;
}

}  // namespace

extern "C" {

int os2rk_abi_version(void) { return OS2R_CMA_ABI_VERSION; }

const char* os2rk_last_error(void) { return g_error.c_str(); }

int os2rk_cma_sample(const Os2rControlLayout* layout, int64_t npops, int32_t nsamples, uint32_t flags, uint64_t seed, uint32_t pop_offset,
                     uint32_t generation, const void* mean_dev, const void* sigma_dev, const void* cov_dev, void* factor_dev,
                     int32_t* failed_dev, void* weights_dev, void* z_dev, void* stream) {
  g_entry_point = "os2rk_cma_sample: ";
  if (const char* why = layout_refusal(layout)) return fail(OS2R_ERR_INVALID, why);
  if (const char* why = shape_refusal(layout, npops, nsamples, flags)) return fail(OS2R_ERR_INVALID, why);
  const uintptr_t elem = layout->dtype == OS2R_F64 ? sizeof(double) : sizeof(float);
  {
    const uintptr_t M = (uintptr_t)npops, SM = (uintptr_t)nsamples * M, E = 2 * ((uintptr_t)layout->obs_dim + 1);
    const Span spans[] = {
        {"mean_dev", mean_dev, M * E * elem, false},
        {"sigma_dev", sigma_dev, M * elem, false},
        {"cov_dev", cov_dev, M * E * E * elem, false},
        {"factor_dev", factor_dev, M * E * E * elem, true},
        {"failed_dev", failed_dev, M * sizeof(int32_t), true},
        {"weights_dev", weights_dev, SM * E * elem, true},
        {"z_dev", z_dev, SM * E * elem, true},
    };
    const int count = sizeof(spans) / sizeof(spans[0]);
    static const char* const optional[] = {"z_dev"};
    std::string why = null_refusal(spans, count, optional, 1);
    if (!why.empty()) return fail(OS2R_ERR_INVALID, why);
    if ((uintptr_t)mean_dev % (2 * elem)) return fail(OS2R_ERR_INVALID, "mean_dev must be aligned to a pair of its elements");
    if ((uintptr_t)weights_dev % (2 * elem)) return fail(OS2R_ERR_INVALID, "weights_dev must be aligned to a pair of its elements");
    if ((uintptr_t)z_dev % (2 * elem)) return fail(OS2R_ERR_INVALID, "z_dev must be aligned to a pair of its elements");
    why = overlap_refusal(spans, count);
    if (!why.empty()) return fail(OS2R_ERR_INVALID, why);
  }
  // the device, from here on
  if (const int rc = check_device(layout->device)) return rc;
  DeviceGuard guard(layout->device);
  auto launch = [&](auto real) {
    using T = decltype(real);
    CmaArgs<T> p;
    std::memset(&p, 0, sizeof(p));
    p.mean = (const T*)mean_dev; p.sigma = (const T*)sigma_dev; p.cov = (const T*)cov_dev; p.factor = (T*)factor_dev; p.failed = failed_dev;
    p.weights = (T*)weights_dev; p.z = (T*)z_dev;
    p.seed = seed; p.M = npops; p.pop_offset = pop_offset; p.generation = generation; p.S = nsamples; p.D = layout->obs_dim;
    launch_cma_sample<T>(p, (hipStream_t)stream);
    return launched(0);
  };
  return layout->dtype == OS2R_F64 ? launch(double()) : launch(float());
}

int os2rk_cma_update(const Os2rControlLayout* layout, int64_t npops, int32_t nsamples, int32_t mu, uint32_t flags, uint64_t seed,
                     uint32_t pop_offset, uint32_t generation, const void* returns_dev, const void* rankw_dev, const void* mean_dev,
                     const void* sigma_dev, const void* cov_dev, const void* p_sigma_dev, const void* p_c_dev, const void* factor_dev,
                     const int32_t* failed_dev, const Os2rkCmaConstants* constants, void* mean_out_dev, void* sigma_out_dev,
                     void* cov_out_dev, void* p_sigma_out_dev, void* p_c_out_dev, int32_t* count_dev, int32_t* status_dev,
                     int32_t* rank_dev, void* yw_dev, void* ps_norm_dev, void* growth_dev, void* stream) {
  g_entry_point = "os2rk_cma_update: ";
  if (const char* why = layout_refusal(layout)) return fail(OS2R_ERR_INVALID, why);
  if (const char* why = shape_refusal(layout, npops, nsamples, flags)) return fail(OS2R_ERR_INVALID, why);
  if (mu < 1) return fail(OS2R_ERR_INVALID, "mu must be >= 1");
  if (mu > nsamples) return fail(OS2R_ERR_INVALID, "mu must be <= nsamples");
  if (!constants) return fail(OS2R_ERR_INVALID, "null constants");
  if (const char* field = constants_refusal(constants)) return fail(OS2R_ERR_INVALID, std::string("constants->") + field + " must be finite");
  const uintptr_t elem = layout->dtype == OS2R_F64 ? sizeof(double) : sizeof(float);
  {
    const uintptr_t M = (uintptr_t)npops, SM = (uintptr_t)nsamples * M, E = 2 * ((uintptr_t)layout->obs_dim + 1);
    const Span spans[] = {
        {"returns_dev", returns_dev, SM * elem, false},
        {"rankw_dev", rankw_dev, (uintptr_t)mu * elem, false},
        {"mean_dev", mean_dev, M * E * elem, false},
        {"sigma_dev", sigma_dev, M * elem, false},
        {"cov_dev", cov_dev, M * E * E * elem, false},
        {"p_sigma_dev", p_sigma_dev, M * E * elem, false},
        {"p_c_dev", p_c_dev, M * E * elem, false},
        {"factor_dev", factor_dev, M * E * E * elem, false},
        {"failed_dev", failed_dev, M * sizeof(int32_t), false},
        {"mean_out_dev", mean_out_dev, M * E * elem, true},
        {"sigma_out_dev", sigma_out_dev, M * elem, true},
        {"cov_out_dev", cov_out_dev, M * E * E * elem, true},
        {"p_sigma_out_dev", p_sigma_out_dev, M * E * elem, true},
        {"p_c_out_dev", p_c_out_dev, M * E * elem, true},
        {"count_dev", count_dev, M * sizeof(int32_t), true},
        {"status_dev", status_dev, M * sizeof(int32_t), true},
        {"rank_dev", rank_dev, SM * sizeof(int32_t), true},
        {"yw_dev", yw_dev, M * E * elem, true},
        {"ps_norm_dev", ps_norm_dev, M * elem, true},
        {"growth_dev", growth_dev, M * elem, true},
    };
    const int count = sizeof(spans) / sizeof(spans[0]);
    static const char* const optional[] = {"yw_dev", "ps_norm_dev", "growth_dev"};
    std::string why = null_refusal(spans, count, optional, 3);
    if (!why.empty()) return fail(OS2R_ERR_INVALID, why);
    if ((uintptr_t)mean_dev % (2 * elem)) return fail(OS2R_ERR_INVALID, "mean_dev must be aligned to a pair of its elements");
    if ((uintptr_t)mean_out_dev % (2 * elem)) return fail(OS2R_ERR_INVALID, "mean_out_dev must be aligned to a pair of its elements");
    if ((uintptr_t)yw_dev % (2 * elem)) return fail(OS2R_ERR_INVALID, "yw_dev must be aligned to a pair of its elements");
    why = overlap_refusal(spans, count);
    if (!why.empty()) return fail(OS2R_ERR_INVALID, why);
  }
  // the device, from here on
  if (const int rc = check_device(layout->device)) return rc;
  DeviceGuard guard(layout->device);
  auto launch = [&](auto real) {
    using T = decltype(real);
    CmaArgs<T> p;
    std::memset(&p, 0, sizeof(p));
    p.returns = (const T*)returns_dev; p.rankw = (const T*)rankw_dev; p.mean = (const T*)mean_dev; p.sigma = (const T*)sigma_dev;
    p.cov = (const T*)cov_dev; p.p_sigma = (const T*)p_sigma_dev; p.p_c = (const T*)p_c_dev; p.factor_in = (const T*)factor_dev;
    p.failed_in = failed_dev;
    p.mean_out = (T*)mean_out_dev; p.sigma_out = (T*)sigma_out_dev; p.cov_out = (T*)cov_out_dev; p.p_sigma_out = (T*)p_sigma_out_dev;
    p.p_c_out = (T*)p_c_out_dev; p.count = count_dev; p.status = status_dev; p.rank = rank_dev; p.yw = (T*)yw_dev;
    p.ps_norm = (T*)ps_norm_dev; p.growth = (T*)growth_dev;
    p.seed = seed; p.M = npops; p.pop_offset = pop_offset; p.generation = generation; p.S = nsamples; p.D = layout->obs_dim; p.mu = mu;
    const Os2rkCmaConstants& k = *constants;
    p.a_sigma = (T)k.a_sigma; p.b_sigma = (T)k.b_sigma; p.hsig_bound = (T)k.hsig_bound; p.a_c = (T)k.a_c; p.b_c = (T)k.b_c;
    p.k0_moving = (T)k.k0_moving; p.k0_stalled = (T)k.k0_stalled; p.c_1 = (T)k.c_1; p.c_mu = (T)k.c_mu; p.g_sigma = (T)k.g_sigma;
    p.chi = (T)k.chi; p.sigma_min = (T)k.sigma_min; p.sigma_max = (T)k.sigma_max;
    launch_cma_update<T>(p, (hipStream_t)stream);
    return launched(0);
  };
  return layout->dtype == OS2R_F64 ? launch(double()) : launch(float());
}

}  // extern "C"
