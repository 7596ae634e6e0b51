// os2r_norm_capi.hip — the C-ABI of libos2r_norm.so (include/os2r_norm.h): the entry points' own argument checks and their
// launches; the check of the layout, the device guard, the gfx950 check and the calling thread's error text are os2r_host.hpp's.
// Every argument check runs before the first HIP call.
#include "os2r_norm.hpp"

// three entry points, three prefixes: each names itself here on entry, and os2r_host.hpp's fail() puts that name in front
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

// what os2rz_obs_stats refuses about the batch's shape, as the refusal's text (null: nothing)
const char* shape_refusal(const Os2rControlLayout* layout, int32_t nsteps, int64_t npolicies, int32_t nsamples, uint32_t flags) {
  if (layout->obs_dim < 1 || layout->obs_dim > OS2R_MAX_OBS) return "layout->obs_dim must be 1..12";
  if (nsteps < 1) return "nsteps must be >= 1";
  if (nsteps > 65535) return "nsteps must be <= 65535";
  if (npolicies < 1) return "npolicies must be >= 1";
  if (nsamples < 1) return "nsamples must be >= 1";
  if (npolicies > 0x7fffffffll / nsamples) return "nsamples * npolicies exceeds 2^31 - 1";
  if (nsamples > 0x7fffffff / nsteps) return "nsamples * nsteps exceeds 2^31 - 1 (the steps of a policy are an int32)";
  if (flags != 0u) return "unknown flag bits";
  return nullptr;
}

// what os2rz_fold and os2rz_unfold refuse about their sets, the scale and the state, as the refusal's text (null: nothing).
// (The double itself is declared free of NaNs: its bits are read back from memory)
const char* sets_refusal(const Os2rControlLayout* layout, int64_t npolicies, int32_t rows, double std_floor, const void* count_dev,
                         const void* mean_dev, const void* m2_dev) {
  if (layout->obs_dim < 1 || layout->obs_dim > OS2R_MAX_OBS) return "layout->obs_dim must be 1..12";
  if (npolicies < 1) return "npolicies must be >= 1";
  if (npolicies > 0x7fffffffll) return "npolicies exceeds 2^31 - 1";
  if (rows != 1 && rows != 2) return "rows must be 1 or 2";
  volatile double mem = std_floor;
  const double v = mem;
  if (!is_finite(&v)) return "std_floor must be finite";
  if (v <= 0.0) return "std_floor must be > 0";
  if (layout->dtype == OS2R_F32 && (float)v == 0.0f) return "std_floor rounds to 0 in the layout's dtype";
  const int given = (count_dev ? 1 : 0) + (mean_dev ? 1 : 0) + (m2_dev ? 1 : 0);
  if (given != 0 && given != 3) return "count_dev, mean_dev and m2_dev must be all null or all given";
  return nullptr;
}

// the launch both of them end in
int fold_launch(const Os2rControlLayout* layout, int64_t npolicies, int64_t nsets, int32_t rows, bool fastest, bool unfold,
                const int64_t* count_dev, const void* mean_dev, const void* m2_dev, double std_floor, const void* in_dev, void* out_dev,
                void* stream) {
  if (const int rc = check_device(layout->device)) return rc;
  DeviceGuard guard(layout->device);
  auto launch = [&](auto real) {
    using T = decltype(real);
    FoldArgs<T> p;
    std::memset(&p, 0, sizeof(p));
    p.count = (const long long*)count_dev; p.mean = (const T*)mean_dev; p.m2 = (const T*)m2_dev;
    p.in = (const T*)in_dev; p.out = (T*)out_dev;
    p.P = npolicies; p.Q = nsets; p.rows = rows; p.D = layout->obs_dim; p.fastest = fastest ? 1 : 0; p.unfold = unfold ? 1 : 0;
    p.floor = (T)std_floor;
    launch_norm_fold<T>(p, (hipStream_t)stream);
    return launched(0);
  };
  return layout->dtype == OS2R_F64 ? launch(double()) : launch(float());
}

}  // namespace

extern "C" {

int os2rz_abi_version(void) { return OS2R_NORM_ABI_VERSION; }

const char* os2rz_last_error(void) { return g_error.c_str(); }

int os2rz_obs_stats(const Os2rControlLayout* layout, int32_t nsteps, int64_t npolicies, int32_t nsamples, uint32_t flags, const void* obs_dev,
                    const void* obs0_dev, const int32_t* length_dev, const int64_t* count_in_dev, const void* mean_in_dev,
                    const void* m2_in_dev, int64_t* count_out_dev, void* mean_out_dev, void* m2_out_dev, int32_t* steps_dev,
                    int32_t* valid_dev, void* lane_sum_dev, int32_t* lane_count_dev, void* stream) {
  g_entry_point = "os2rz_obs_stats: ";
  if (const char* why = layout_refusal(layout)) return fail(OS2R_ERR_INVALID, why);
  if (const char* why = shape_refusal(layout, nsteps, npolicies, nsamples, flags)) return fail(OS2R_ERR_INVALID, why);
  if (!obs_dev) return fail(OS2R_ERR_INVALID, "null obs_dev");
  {
    const int given = (count_in_dev ? 1 : 0) + (mean_in_dev ? 1 : 0) + (m2_in_dev ? 1 : 0);
    if (given != 0 && given != 3) return fail(OS2R_ERR_INVALID, "count_in_dev, mean_in_dev and m2_in_dev must be all null or all given");
  }
  if (!count_out_dev) return fail(OS2R_ERR_INVALID, "null count_out_dev");
  if (!mean_out_dev) return fail(OS2R_ERR_INVALID, "null mean_out_dev");
  if (!m2_out_dev) return fail(OS2R_ERR_INVALID, "null m2_out_dev");
  if (!lane_sum_dev) return fail(OS2R_ERR_INVALID, "null lane_sum_dev (the second launch reads it)");
  if (!lane_count_dev) return fail(OS2R_ERR_INVALID, "null lane_count_dev (the second launch reads it)");
  const uintptr_t elem = layout->dtype == OS2R_F64 ? sizeof(double) : sizeof(float);
  {
    const uintptr_t K = (uintptr_t)nsteps, P = (uintptr_t)npolicies, N = (uintptr_t)nsamples * P, D = (uintptr_t)layout->obs_dim;
    const Span spans[] = {
        {"obs_dev", obs_dev, K * N * D * elem, false},
        {"obs0_dev", obs0_dev, N * D * elem, false},
        {"length_dev", length_dev, N * sizeof(int32_t), false},
        {"count_in_dev", count_in_dev, P * sizeof(int64_t), false},
        {"mean_in_dev", mean_in_dev, P * D * elem, false},
        {"m2_in_dev", m2_in_dev, P * D * elem, false},
        {"count_out_dev", count_out_dev, P * sizeof(int64_t), true},
        {"mean_out_dev", mean_out_dev, P * D * elem, true},
        {"m2_out_dev", m2_out_dev, P * D * elem, true},
        {"steps_dev", steps_dev, P * sizeof(int32_t), true},
        {"valid_dev", valid_dev, P * sizeof(int32_t), true},
        {"lane_sum_dev", lane_sum_dev, 2 * D * N * elem, true},
        {"lane_count_dev", lane_count_dev, OS2RZ_LANE_COUNTS * N * sizeof(int32_t), true},
    };
    const std::string why = overlap_refusal(spans, sizeof(spans) / sizeof(spans[0]));
    if (!why.empty()) return fail(OS2R_ERR_INVALID, why);
  }
  // the device, from here on
  if (const int rc = check_device(layout->device)) return rc;
  DeviceGuard guard(layout->device);
  auto launch = [&](auto real) {
    using T = decltype(real);
    StatsArgs<T> p;
    std::memset(&p, 0, sizeof(p));
    p.obs = (const T*)obs_dev; p.obs0 = (const T*)obs0_dev; p.length = length_dev;
    p.count_in = (const long long*)count_in_dev; p.mean_in = (const T*)mean_in_dev; p.m2_in = (const T*)m2_in_dev;
    p.count_out = (long long*)count_out_dev; p.mean_out = (T*)mean_out_dev; p.m2_out = (T*)m2_out_dev;
    p.steps = steps_dev; p.valid = valid_dev; p.lane_sum = (T*)lane_sum_dev; p.lane_count = lane_count_dev;
    p.P = npolicies; p.N = (long long)nsamples * npolicies; p.K = nsteps; p.S = nsamples; p.D = layout->obs_dim;
    p.lanes_per_block = kNormBlock / layout->obs_dim;
    launch_obs_stats<T>(p, (hipStream_t)stream);
    return launched(0);
  };
  return layout->dtype == OS2R_F64 ? launch(double()) : launch(float());
}

int os2rz_fold(const Os2rControlLayout* layout, int64_t npolicies, int64_t nlanes, int32_t rows, uint32_t flags, const int64_t* count_dev,
               const void* mean_dev, const void* m2_dev, double std_floor, const void* theta_dev, void* weights_dev, void* stream) {
  g_entry_point = "os2rz_fold: ";
  if (const char* why = layout_refusal(layout)) return fail(OS2R_ERR_INVALID, why);
  if (const char* why = sets_refusal(layout, npolicies, rows, std_floor, count_dev, mean_dev, m2_dev)) return fail(OS2R_ERR_INVALID, why);
  if (flags & ~(OS2RZ_PER_LANE | OS2RZ_POLICY_FASTEST)) return fail(OS2R_ERR_INVALID, "unknown flag bits");
  const bool per_lane = (flags & OS2RZ_PER_LANE) != 0u;
  if (per_lane && nlanes < 1) return fail(OS2R_ERR_INVALID, "nlanes must be >= 1 with OS2RZ_PER_LANE");
  if (per_lane && nlanes > 0x7fffffffll) return fail(OS2R_ERR_INVALID, "nlanes exceeds 2^31 - 1");
  if (per_lane && nlanes % npolicies) return fail(OS2R_ERR_INVALID, "nlanes must be a multiple of npolicies (lane l is under policy l mod npolicies)");
  if (!theta_dev) return fail(OS2R_ERR_INVALID, "null theta_dev");
  if (!weights_dev) return fail(OS2R_ERR_INVALID, "null weights_dev");
  const int64_t nsets = per_lane ? nlanes : npolicies;
  {
    const uintptr_t elem = layout->dtype == OS2R_F64 ? sizeof(double) : sizeof(float);
    const uintptr_t P = (uintptr_t)npolicies, D = (uintptr_t)layout->obs_dim, E = (uintptr_t)nsets * (uintptr_t)rows * (D + 1);
    const Span spans[] = {
        {"count_dev", count_dev, P * sizeof(int64_t), false},
        {"mean_dev", mean_dev, P * D * elem, false},
        {"m2_dev", m2_dev, P * D * elem, false},
        {"theta_dev", theta_dev, E * elem, false},
        {"weights_dev", weights_dev, E * elem, true},
    };
    const std::string why = overlap_refusal(spans, sizeof(spans) / sizeof(spans[0]));
    if (!why.empty()) return fail(OS2R_ERR_INVALID, why);
  }
  // the device, from here on
  return fold_launch(layout, npolicies, nsets, rows, (flags & OS2RZ_POLICY_FASTEST) != 0u, false, count_dev, mean_dev, m2_dev, std_floor,
                     theta_dev, weights_dev, stream);
}

int os2rz_unfold(const Os2rControlLayout* layout, int64_t npolicies, int32_t rows, uint32_t flags, const int64_t* count_dev,
                 const void* mean_dev, const void* m2_dev, double std_floor, const void* grad_dev, void* grad_theta_dev, void* stream) {
  g_entry_point = "os2rz_unfold: ";
  if (const char* why = layout_refusal(layout)) return fail(OS2R_ERR_INVALID, why);
  if (const char* why = sets_refusal(layout, npolicies, rows, std_floor, count_dev, mean_dev, m2_dev)) return fail(OS2R_ERR_INVALID, why);
  if (flags & OS2RZ_PER_LANE) return fail(OS2R_ERR_INVALID, "OS2RZ_PER_LANE is os2rz_fold's (a gradient is per policy)");
  if (flags & ~OS2RZ_POLICY_FASTEST) return fail(OS2R_ERR_INVALID, "unknown flag bits");
  if (!grad_dev) return fail(OS2R_ERR_INVALID, "null grad_dev");
  if (!grad_theta_dev) return fail(OS2R_ERR_INVALID, "null grad_theta_dev");
  {
    const uintptr_t elem = layout->dtype == OS2R_F64 ? sizeof(double) : sizeof(float);
    const uintptr_t P = (uintptr_t)npolicies, D = (uintptr_t)layout->obs_dim, E = P * (uintptr_t)rows * (D + 1);
    const Span spans[] = {
        {"count_dev", count_dev, P * sizeof(int64_t), false},
        {"mean_dev", mean_dev, P * D * elem, false},
        {"m2_dev", m2_dev, P * D * elem, false},
        {"grad_dev", grad_dev, E * elem, false},
        {"grad_theta_dev", grad_theta_dev, E * elem, true},
    };
    const std::string why = overlap_refusal(spans, sizeof(spans) / sizeof(spans[0]));
    if (!why.empty()) return fail(OS2R_ERR_INVALID, why);
  }
  // the device, from here on
  return fold_launch(layout, npolicies, npolicies, rows, (flags & OS2RZ_POLICY_FASTEST) != 0u, true, count_dev, mean_dev, m2_dev, std_floor,
                     grad_dev, grad_theta_dev, stream);
}

}  // extern "C"
