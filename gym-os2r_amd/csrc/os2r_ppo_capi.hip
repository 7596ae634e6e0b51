// os2r_ppo_capi.hip — the C-ABI of libos2r_ppo.so (include/os2r_ppo.h): the entry point's own argument checks and the two launches;
// the check of the layout, the device guard, the gfx950 check and the calling thread's error text are os2r_host.hpp's.
// Every argument check runs before the first HIP call.
#include "os2r_ppo.hpp"

#define OS2R_HOST_ERROR_PREFIX "os2ro_ppo_gradient: "
#include "os2r_host.hpp"

using namespace os2r;

namespace {

// one device array of the call: [at, at + bytes)
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

}  // namespace

extern "C" {

int os2ro_abi_version(void) { return OS2R_PPO_ABI_VERSION; }

const char* os2ro_last_error(void) { return g_error.c_str(); }

int os2ro_ppo_gradient(const Os2rControlLayout* layout, int32_t nsteps, int64_t npolicies, int32_t nsamples, uint32_t flags,
                       const void* obs_dev, const void* obs0_dev, const void* noise_dev, const void* action_dev, const void* sigma_dev,
                       const void* sigma_new_dev, const void* weight_dev, const void* weight_old_dev, const int32_t* length_dev,
                       const void* adv_dev, double clip, void* grad_dev, void* lane_grad_dev, void* lsig_grad_dev, void* lane_lsig_dev,
                       void* stat_dev, void* lane_stat_dev, int32_t* steps_dev, int32_t* clipped_dev, int32_t* gated_dev, int32_t* valid_dev,
                       void* ratio_dev, int32_t* lane_count_dev, void* stream) {
  if (const char* why = layout_refusal(layout)) return fail(OS2R_ERR_INVALID, why);
  if (layout->obs_dim < 1 || layout->obs_dim > OS2R_MAX_OBS) return fail(OS2R_ERR_INVALID, "layout->obs_dim must be 1..12");
  if (nsteps < 1) return fail(OS2R_ERR_INVALID, "nsteps must be >= 1");
  if (nsteps > 65535) return fail(OS2R_ERR_INVALID, "nsteps must be <= 65535");
  if (npolicies < 1) return fail(OS2R_ERR_INVALID, "npolicies must be >= 1");
  if (nsamples < 1) return fail(OS2R_ERR_INVALID, "nsamples must be >= 1");
  if (npolicies > 0x7fffffffll / nsamples) return fail(OS2R_ERR_INVALID, "nsamples * npolicies exceeds 2^31 - 1");
  if (nsamples > 0x7fffffff / nsteps) return fail(OS2R_ERR_INVALID, "nsamples * nsteps exceeds 2^31 - 1 (the steps of a policy are an int32)");
  if (flags & ~(uint32_t)(OS2RO_TANH | OS2RO_SIGMA_PER_LANE)) return fail(OS2R_ERR_INVALID, "unknown flag bits");
  double lo, hi;
  {
    // (the argument itself is declared free of NaNs: its bits are read back from memory)
    volatile double mem = clip;
    const double c = mem;
    if (!is_finite(&c)) return fail(OS2R_ERR_INVALID, "clip must be finite");
    if (c <= 0.0 || c >= 1.0) return fail(OS2R_ERR_INVALID, "clip must be in (0, 1)");
    lo = 1.0 - c;
    hi = 1.0 + c;
  }
  const bool tanh = (flags & OS2RO_TANH) != 0, per_lane = (flags & OS2RO_SIGMA_PER_LANE) != 0;
  if (!obs_dev) return fail(OS2R_ERR_INVALID, "null obs_dev");
  if (!noise_dev) return fail(OS2R_ERR_INVALID, "null noise_dev");
  if (!sigma_dev) return fail(OS2R_ERR_INVALID, "null sigma_dev");
  if (!weight_dev) return fail(OS2R_ERR_INVALID, "null weight_dev");
  if (!weight_old_dev) return fail(OS2R_ERR_INVALID, "null weight_old_dev");
  if (!adv_dev) return fail(OS2R_ERR_INVALID, "null adv_dev");
  if (!grad_dev) return fail(OS2R_ERR_INVALID, "null grad_dev");
  if (!lane_grad_dev) return fail(OS2R_ERR_INVALID, "null lane_grad_dev");
  if (!lane_stat_dev) return fail(OS2R_ERR_INVALID, "null lane_stat_dev");
  if (!lane_count_dev) return fail(OS2R_ERR_INVALID, "null lane_count_dev");
  if (!tanh && !action_dev) return fail(OS2R_ERR_INVALID, "null action_dev without OS2RO_TANH");
  if (lsig_grad_dev && !lane_lsig_dev) return fail(OS2R_ERR_INVALID, "lsig_grad_dev needs lane_lsig_dev");
  if (lane_lsig_dev && !lsig_grad_dev) return fail(OS2R_ERR_INVALID, "lane_lsig_dev needs lsig_grad_dev");
  const uintptr_t elem = layout->dtype == OS2R_F64 ? sizeof(double) : sizeof(float);
  if ((uintptr_t)noise_dev % (2 * elem)) return fail(OS2R_ERR_INVALID, "noise_dev must be aligned to a pair of its elements");
  if (!tanh && (uintptr_t)action_dev % (2 * elem)) return fail(OS2R_ERR_INVALID, "action_dev must be aligned to a pair of its elements");
  {
    const uintptr_t K = (uintptr_t)nsteps, P = (uintptr_t)npolicies, N = (uintptr_t)nsamples * P, D = (uintptr_t)layout->obs_dim;
    const Span spans[] = {
        {"obs_dev", obs_dev, K * N * D * elem, false},
        {"obs0_dev", obs0_dev, N * D * elem, false},
        {"noise_dev", noise_dev, K * N * 2 * elem, false},
        {"action_dev", tanh ? nullptr : action_dev, K * N * 2 * elem, false},
        {"sigma_dev", sigma_dev, (per_lane ? 2 * N : 2) * elem, false},
        {"sigma_new_dev", sigma_new_dev, 2 * P * elem, false},
        {"weight_dev", weight_dev, 2 * (D + 1) * P * elem, false},
        {"weight_old_dev", weight_old_dev, 2 * (D + 1) * P * elem, false},
        {"length_dev", length_dev, N * sizeof(int32_t), false},
        {"adv_dev", adv_dev, K * N * elem, false},
        {"grad_dev", grad_dev, 2 * (D + 1) * P * elem, true},
        {"lane_grad_dev", lane_grad_dev, 2 * (D + 1) * N * elem, true},
        {"lsig_grad_dev", lsig_grad_dev, 2 * P * elem, true},
        {"lane_lsig_dev", lane_lsig_dev, 2 * N * elem, true},
        {"stat_dev", stat_dev, OS2RO_STATS * P * elem, true},
        {"lane_stat_dev", lane_stat_dev, OS2RO_STATS * N * elem, true},
        {"steps_dev", steps_dev, P * sizeof(int32_t), true},
        {"clipped_dev", clipped_dev, 2 * P * sizeof(int32_t), true},
        {"gated_dev", gated_dev, P * sizeof(int32_t), true},
        {"valid_dev", valid_dev, P * sizeof(int32_t), true},
        {"ratio_dev", ratio_dev, K * N * elem, true},
        {"lane_count_dev", lane_count_dev, OS2RO_LANE_COUNTS * N * sizeof(int32_t), true},
    };
    constexpr int count = sizeof(spans) / sizeof(spans[0]);
    for (int o = 0; o < count; ++o)                       // every output against every input and every output before it
      for (int i = 0; spans[o].output && spans[o].at && i < o; ++i)
        if (spans[i].at && overlap(spans[o], spans[i])) return fail(OS2R_ERR_INVALID, std::string(spans[o].name) + " overlaps " + spans[i].name);
  }
  // the device, from here on
  if (const int rc = check_device(layout->device)) return rc;
  DeviceGuard guard(layout->device);
  auto launch = [&](auto real) {
    using T = decltype(real);
    PpoArgs<T> p;
    std::memset(&p, 0, sizeof(p));
    p.obs = (const T*)obs_dev; p.obs0 = (const T*)obs0_dev; p.noise = (const T*)noise_dev; p.action = tanh ? nullptr : (const T*)action_dev;
    p.sigma = (const T*)sigma_dev; p.sigma_new = (const T*)sigma_new_dev; p.weight = (const T*)weight_dev;
    p.weight_old = (const T*)weight_old_dev; p.length = length_dev; p.adv = (const T*)adv_dev;
    p.grad = (T*)grad_dev; p.lane_grad = (T*)lane_grad_dev; p.lsig_grad = (T*)lsig_grad_dev; p.lane_lsig = (T*)lane_lsig_dev;
    p.stat = (T*)stat_dev; p.lane_stat = (T*)lane_stat_dev; p.steps = steps_dev; p.clipped = clipped_dev; p.gated = gated_dev;
    p.valid = valid_dev; p.ratio = (T*)ratio_dev; p.lane_count = lane_count_dev;
    p.P = npolicies; p.N = (long long)nsamples * npolicies; p.K = nsteps; p.S = nsamples; p.D = layout->obs_dim;
    p.tanh = tanh ? 1 : 0; p.sigma_per_lane = per_lane ? 1 : 0;
    p.lo = (T)lo; p.hi = (T)hi;
    launch_ppo_gradient<T>(p, (hipStream_t)stream);
    return launched(0);
  };
  return layout->dtype == OS2R_F64 ? launch(double()) : launch(float());
}

}  // extern "C"
