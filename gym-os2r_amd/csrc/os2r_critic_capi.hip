// os2r_critic_capi.hip — the C-ABI of libos2r_critic.so (include/os2r_critic.h): the entry points' own argument checks and their
// launches; the check of the layout, the device guard, the gfx950 check and the calling thread's error text are os2r_host.hpp's.
// Every argument check runs before the first HIP call.
#include "os2r_critic.hpp"

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

// what both entry points refuse about the batch's shape, as the refusal's text (null: nothing)
const char* shape_refusal(const Os2rControlLayout* layout, int32_t nsteps, int64_t npolicies, int32_t nsamples) {
  if (layout->obs_dim < 1 || layout->obs_dim > OS2R_MAX_OBS) return "layout->obs_dim must be 1..12";
  if (nsteps < 1) return "nsteps must be >= 1";
  if (nsteps > 65535) return "nsteps must be <= 65535";
  if (npolicies < 1) return "npolicies must be >= 1";
  if (nsamples < 1) return "nsamples must be >= 1";
  if (npolicies > 0x7fffffffll / nsamples) return "nsamples * npolicies exceeds 2^31 - 1";
  if (nsamples > 0x7fffffff / nsteps) return "nsamples * nsteps exceeds 2^31 - 1 (the steps of a policy are an int32)";
  return nullptr;
}

// 0: fine; 1: not finite; 2: outside [lo, hi].  (The argument itself is declared free of NaNs: its bits are read back from memory)
int range_refusal(double value, double lo, double hi) {
  volatile double mem = value;
  const double v = mem;
  if (!is_finite(&v)) return 1;
  return v < lo || v > hi ? 2 : 0;
}

}  // namespace

extern "C" {

int os2rv_abi_version(void) { return OS2R_CRITIC_ABI_VERSION; }

const char* os2rv_last_error(void) { return g_error.c_str(); }

int os2rv_gae(const Os2rControlLayout* layout, int32_t nsteps, int64_t npolicies, int32_t nsamples, const void* obs_dev, const void* obs0_dev,
              const void* term_obs_dev, const void* reward_dev, const uint8_t* done_dev, const int32_t* length_dev, const void* value_w_dev,
              double gamma, double lambda, void* adv_dev, void* ret_dev, void* value_dev, void* stream) {
  g_entry_point = "os2rv_gae: ";
  if (const char* why = layout_refusal(layout)) return fail(OS2R_ERR_INVALID, why);
  if (const char* why = shape_refusal(layout, nsteps, npolicies, nsamples)) return fail(OS2R_ERR_INVALID, why);
  if (const int bad = range_refusal(gamma, 0.0, 1.0)) return fail(OS2R_ERR_INVALID, bad == 1 ? "gamma must be finite" : "gamma must be in [0, 1]");
  if (const int bad = range_refusal(lambda, 0.0, 1.0)) return fail(OS2R_ERR_INVALID, bad == 1 ? "lambda must be finite" : "lambda must be in [0, 1]");
  if (!obs_dev) return fail(OS2R_ERR_INVALID, "null obs_dev");
  if (!obs0_dev) return fail(OS2R_ERR_INVALID, "null obs0_dev (the knot-observation form is out of scope)");
  if (!reward_dev) return fail(OS2R_ERR_INVALID, "null reward_dev");
  if (!done_dev) return fail(OS2R_ERR_INVALID, "null done_dev");
  if (!value_w_dev) return fail(OS2R_ERR_INVALID, "null value_w_dev");
  if (!adv_dev) return fail(OS2R_ERR_INVALID, "null adv_dev");
  if (!value_dev) return fail(OS2R_ERR_INVALID, "null value_dev (the second launch reads it)");
  const uintptr_t elem = layout->dtype == OS2R_F64 ? sizeof(double) : sizeof(float);
  {
    const uintptr_t K = (uintptr_t)nsteps, P = (uintptr_t)npolicies, N = (uintptr_t)nsamples * P, D = (uintptr_t)layout->obs_dim;
    const Span spans[] = {
        {"obs_dev", obs_dev, K * N * D * elem, false},
        {"obs0_dev", obs0_dev, N * D * elem, false},
        {"term_obs_dev", term_obs_dev, K * N * D * elem, false},
        {"reward_dev", reward_dev, K * N * elem, false},
        {"done_dev", done_dev, K * N, false},
        {"length_dev", length_dev, N * sizeof(int32_t), false},
        {"value_w_dev", value_w_dev, (D + 1) * P * elem, false},
        {"adv_dev", adv_dev, K * N * elem, true},
        {"ret_dev", ret_dev, K * N * elem, true},
        {"value_dev", value_dev, K * N * elem, true},
    };
    const std::string why = overlap_refusal(spans, sizeof(spans) / sizeof(spans[0]));
    if (!why.empty()) return fail(OS2R_ERR_INVALID, why);
  }
  // the device, from here on
  if (const int rc = check_device(layout->device)) return rc;
  DeviceGuard guard(layout->device);
  auto launch = [&](auto real) {
    using T = decltype(real);
    GaeArgs<T> p;
    std::memset(&p, 0, sizeof(p));
    p.obs = (const T*)obs_dev; p.obs0 = (const T*)obs0_dev; p.term_obs = (const T*)term_obs_dev; p.reward = (const T*)reward_dev;
    p.done = done_dev; p.length = length_dev; p.value_w = (const T*)value_w_dev;
    p.adv = (T*)adv_dev; p.ret = (T*)ret_dev; p.value = (T*)value_dev;
    p.P = npolicies; p.N = (long long)nsamples * npolicies; p.K = nsteps; p.D = layout->obs_dim;
    p.gamma = (T)gamma;
    {
#pragma clang fp contract(off)
      const volatile T lam = (T)lambda;                 // c = gamma lambda: one product of the two rounded values, in T
      p.c = p.gamma * lam;
    }
    launch_gae<T>(p, (hipStream_t)stream);
    return launched(0);
  };
  return layout->dtype == OS2R_F64 ? launch(double()) : launch(float());
}

int os2rv_value_fit(const Os2rControlLayout* layout, int32_t nsteps, int64_t npolicies, int32_t nsamples, const void* obs_dev,
                    const void* obs0_dev, const void* target_dev, const int32_t* length_dev, const void* prev_w_dev, double ridge, void* w_dev,
                    void* lane_mom_dev, void* mom_dev, int32_t* lane_count_dev, int32_t* failed_dev, int32_t* steps_dev, int32_t* valid_dev,
                    void* stream) {
  g_entry_point = "os2rv_value_fit: ";
  if (const char* why = layout_refusal(layout)) return fail(OS2R_ERR_INVALID, why);
  if (const char* why = shape_refusal(layout, nsteps, npolicies, nsamples)) return fail(OS2R_ERR_INVALID, why);
  if (const int bad = range_refusal(ridge, 0.0, 1.7976931348623157e308)) return fail(OS2R_ERR_INVALID, bad == 1 ? "ridge must be finite" : "ridge must be >= 0");
  if (!obs_dev) return fail(OS2R_ERR_INVALID, "null obs_dev");
  if (!obs0_dev) return fail(OS2R_ERR_INVALID, "null obs0_dev (the knot-observation form is out of scope)");
  if (!target_dev) return fail(OS2R_ERR_INVALID, "null target_dev");
  if (!w_dev) return fail(OS2R_ERR_INVALID, "null w_dev");
  if (!lane_mom_dev) return fail(OS2R_ERR_INVALID, "null lane_mom_dev (the second launch reads it)");
  if (!mom_dev) return fail(OS2R_ERR_INVALID, "null mom_dev (the third launch reads it)");
  if (!lane_count_dev) return fail(OS2R_ERR_INVALID, "null lane_count_dev (the second launch reads it)");
  const uintptr_t elem = layout->dtype == OS2R_F64 ? sizeof(double) : sizeof(float);
  {
    const uintptr_t K = (uintptr_t)nsteps, P = (uintptr_t)npolicies, N = (uintptr_t)nsamples * P, D = (uintptr_t)layout->obs_dim;
    const uintptr_t E = (D + 1) * (D + 2) / 2 + (D + 1);
    const Span spans[] = {
        {"obs_dev", obs_dev, K * N * D * elem, false},
        {"obs0_dev", obs0_dev, N * D * elem, false},
        {"target_dev", target_dev, K * N * elem, false},
        {"length_dev", length_dev, N * sizeof(int32_t), false},
        {"prev_w_dev", prev_w_dev, (D + 1) * P * elem, false},
        {"w_dev", w_dev, (D + 1) * P * elem, true},
        {"lane_mom_dev", lane_mom_dev, E * N * elem, true},
        {"mom_dev", mom_dev, E * P * elem, true},
        {"lane_count_dev", lane_count_dev, OS2RV_LANE_COUNTS * N * sizeof(int32_t), true},
        {"failed_dev", failed_dev, P * sizeof(int32_t), true},
        {"steps_dev", steps_dev, P * sizeof(int32_t), true},
        {"valid_dev", valid_dev, P * sizeof(int32_t), true},
    };
    const std::string why = overlap_refusal(spans, sizeof(spans) / sizeof(spans[0]));
    if (!why.empty()) return fail(OS2R_ERR_INVALID, why);
  }
  // the device, from here on
  if (const int rc = check_device(layout->device)) return rc;
  DeviceGuard guard(layout->device);
  auto launch = [&](auto real) {
    using T = decltype(real);
    FitArgs<T> p;
    std::memset(&p, 0, sizeof(p));
    p.obs = (const T*)obs_dev; p.obs0 = (const T*)obs0_dev; p.target = (const T*)target_dev; p.length = length_dev;
    p.prev_w = (const T*)prev_w_dev; p.w = (T*)w_dev; p.lane_mom = (T*)lane_mom_dev; p.mom = (T*)mom_dev;
    p.lane_count = lane_count_dev; p.failed = failed_dev; p.steps = steps_dev; p.valid = valid_dev;
    p.P = npolicies; p.N = (long long)nsamples * npolicies; p.K = nsteps; p.S = nsamples; p.D = layout->obs_dim;
    p.ridge = (T)ridge;                                  // (a ridge above the dtype's largest number rounds to infinity: every factor fails)
    launch_value_fit<T>(p, (hipStream_t)stream);
    return launched(0);
  };
  return layout->dtype == OS2R_F64 ? launch(double()) : launch(float());
}

}  // extern "C"
