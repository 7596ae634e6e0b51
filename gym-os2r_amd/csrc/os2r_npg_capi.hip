// os2r_npg_capi.hip — the C-ABI of libos2r_npg.so (include/os2r_npg.h): the entry point's own argument checks and the three launches;
// the check of the layout, the device guard, the gfx950 check and the calling thread's error text are os2r_host.hpp's.
// Every argument check runs before the first HIP call.
#include "os2r_npg.hpp"

#define OS2R_HOST_ERROR_PREFIX "os2rn_natural_step: "
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

int os2rn_abi_version(void) { return OS2R_NPG_ABI_VERSION; }

const char* os2rn_last_error(void) { return g_error.c_str(); }

int os2rn_natural_step(const Os2rControlLayout* layout, int32_t nsteps, int64_t npolicies, int32_t nsamples, uint32_t flags,
                       const void* obs_dev, const void* obs0_dev, const void* action_dev, const void* sigma_dev, const int32_t* length_dev,
                       const void* grad_dev, const void* lsig_grad_dev, double damping, double kl, void* step_dev, void* dir_dev,
                       void* lsig_step_dev, void* beta_dev, void* quad_dev, int32_t* failed_dev, int32_t* steps_dev, int32_t* open_dev,
                       int32_t* valid_dev, void* lane_mom_dev, void* mom_dev, int32_t* lane_count_dev, void* stream) {
  if (const char* why = layout_refusal(layout)) return fail(OS2R_ERR_INVALID, why);
  if (layout->obs_dim < 1 || layout->obs_dim > OS2R_MAX_OBS) return fail(OS2R_ERR_INVALID, "layout->obs_dim must be 1..12");
  if (nsteps < 1) return fail(OS2R_ERR_INVALID, "nsteps must be >= 1");
  if (nsteps > 65535) return fail(OS2R_ERR_INVALID, "nsteps must be <= 65535");
  if (npolicies < 1) return fail(OS2R_ERR_INVALID, "npolicies must be >= 1");
  if (nsamples < 1) return fail(OS2R_ERR_INVALID, "nsamples must be >= 1");
  if (npolicies > 0x7fffffffll / nsamples) return fail(OS2R_ERR_INVALID, "nsamples * npolicies exceeds 2^31 - 1");
  if (nsamples > 0x7fffffff / nsteps) return fail(OS2R_ERR_INVALID, "nsamples * nsteps exceeds 2^31 - 1 (the steps of a policy are an int32)");
  if (flags & ~(uint32_t)(OS2RN_TANH | OS2RN_SIGMA_PER_LANE)) return fail(OS2R_ERR_INVALID, "unknown flag bits");
  double damp, bound;
  {
    // (the arguments themselves are declared free of NaNs: their bits are read back from memory)
    volatile double mem_d = damping, mem_k = kl;
    damp = mem_d;
    bound = mem_k;
    if (!is_finite(&damp)) return fail(OS2R_ERR_INVALID, "damping must be finite");
    if (damp < 0.0) return fail(OS2R_ERR_INVALID, "damping must be >= 0");
    if (!is_finite(&bound)) return fail(OS2R_ERR_INVALID, "kl must be finite");
    if (bound < 0.0) return fail(OS2R_ERR_INVALID, "kl must be >= 0");
  }
  const bool tanh = (flags & OS2RN_TANH) != 0, per_lane = (flags & OS2RN_SIGMA_PER_LANE) != 0;
  if (!obs_dev) return fail(OS2R_ERR_INVALID, "null obs_dev");
  if (!sigma_dev) return fail(OS2R_ERR_INVALID, "null sigma_dev");
  if (!grad_dev) return fail(OS2R_ERR_INVALID, "null grad_dev");
  if (!step_dev) return fail(OS2R_ERR_INVALID, "null step_dev");
  if (!lane_mom_dev) return fail(OS2R_ERR_INVALID, "null lane_mom_dev");
  if (!mom_dev) return fail(OS2R_ERR_INVALID, "null mom_dev");
  if (!lane_count_dev) return fail(OS2R_ERR_INVALID, "null lane_count_dev");
  if (!tanh && !action_dev) return fail(OS2R_ERR_INVALID, "null action_dev without OS2RN_TANH");
  if (lsig_step_dev && !lsig_grad_dev) return fail(OS2R_ERR_INVALID, "lsig_step_dev needs lsig_grad_dev");
  if (lsig_grad_dev && !lsig_step_dev) return fail(OS2R_ERR_INVALID, "lsig_grad_dev needs lsig_step_dev");
  const uintptr_t elem = layout->dtype == OS2R_F64 ? sizeof(double) : sizeof(float);
  if (!tanh && (uintptr_t)action_dev % (2 * elem)) return fail(OS2R_ERR_INVALID, "action_dev must be aligned to a pair of its elements");
  {
    const uintptr_t K = (uintptr_t)nsteps, P = (uintptr_t)npolicies, N = (uintptr_t)nsamples * P, D = (uintptr_t)layout->obs_dim;
    const uintptr_t E = (D + 1) * (D + 2);                // 2 Tri
    const Span spans[] = {
        {"obs_dev", obs_dev, K * N * D * elem, false},
        {"obs0_dev", obs0_dev, N * D * elem, false},
        {"action_dev", tanh ? nullptr : action_dev, K * N * 2 * elem, false},
        {"sigma_dev", sigma_dev, (per_lane ? 2 * N : 2) * elem, false},
        {"length_dev", length_dev, N * sizeof(int32_t), false},
        {"grad_dev", grad_dev, 2 * (D + 1) * P * elem, false},
        {"lsig_grad_dev", lsig_grad_dev, 2 * P * elem, false},
        {"step_dev", step_dev, 2 * (D + 1) * P * elem, true},
        {"dir_dev", dir_dev, 2 * (D + 1) * P * elem, true},
        {"lsig_step_dev", lsig_step_dev, 2 * P * elem, true},
        {"beta_dev", beta_dev, P * elem, true},
        {"quad_dev", quad_dev, P * elem, true},
        {"failed_dev", failed_dev, 3 * P * sizeof(int32_t), true},
        {"steps_dev", steps_dev, P * sizeof(int32_t), true},
        {"open_dev", open_dev, 2 * P * sizeof(int32_t), true},
        {"valid_dev", valid_dev, P * sizeof(int32_t), true},
        {"lane_mom_dev", lane_mom_dev, E * N * elem, true},
        {"mom_dev", mom_dev, E * P * elem, true},
        {"lane_count_dev", lane_count_dev, OS2RN_LANE_COUNTS * N * sizeof(int32_t), true},
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
    NpgArgs<T> p;
    std::memset(&p, 0, sizeof(p));
    p.obs = (const T*)obs_dev; p.obs0 = (const T*)obs0_dev; p.action = tanh ? nullptr : (const T*)action_dev;
    p.sigma = (const T*)sigma_dev; p.length = length_dev; p.grad = (const T*)grad_dev; p.lsig_grad = (const T*)lsig_grad_dev;
    p.step = (T*)step_dev; p.dir = (T*)dir_dev; p.lsig_step = (T*)lsig_step_dev; p.beta = (T*)beta_dev; p.quad = (T*)quad_dev;
    p.failed = failed_dev; p.steps = steps_dev; p.open = open_dev; p.valid = valid_dev;
    p.lane_mom = (T*)lane_mom_dev; p.mom = (T*)mom_dev; p.lane_count = lane_count_dev;
    p.P = npolicies; p.N = (long long)nsamples * npolicies; p.K = nsteps; p.S = nsamples; p.D = layout->obs_dim;
    p.tanh = tanh ? 1 : 0; p.sigma_per_lane = per_lane ? 1 : 0;
    p.unit = bound == 0.0 ? 1 : 0;
    p.damping = (T)damp; p.kl = (T)bound;
    launch_natural_step<T>(p, (hipStream_t)stream);
    return launched(0);
  };
  return layout->dtype == OS2R_F64 ? launch(double()) : launch(float());
}

}  // extern "C"
