// os2r_es_capi.hip — the C-ABI of libos2r_es.so (include/os2r_es.h): the entry points' own argument checks and their launches;
// the check of the layout, the device guard, the gfx950 check and the calling thread's error text are os2r_host.hpp's.
// Every argument check runs before the first HIP call.
#include "os2r_es.hpp"

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

// what both entry points refuse about the populations' shape, as the refusal's text (null: nothing)
const char* shape_refusal(const Os2rControlLayout* layout, int64_t npops, int32_t ndirs, uint32_t flags) {
  if (layout->obs_dim < 1 || layout->obs_dim > OS2R_MAX_OBS) return "layout->obs_dim must be 1..12";
  if (npops < 1) return "npops must be >= 1";
  if (ndirs < 1) return "ndirs must be >= 1";
  if (ndirs > OS2RA_MAX_DIRECTIONS) return "ndirs must be < 2^27 (16 ndirs is a 32-bit counter word)";
  if (npops > 0x7fffffffll / 2 / ndirs) return "2 * ndirs * npops exceeds 2^31 - 1";
  if (flags != 0u) return "unknown flag bits";
  return nullptr;
}

// 0: fine; 1: not finite; 2: negative.  (The argument itself is declared free of NaNs: its bits are read back from memory)
int scale_refusal(double value) {
  volatile double mem = value;
  const double v = mem;
  if (!is_finite(&v)) return 1;
  return v < 0.0 ? 2 : 0;
}

}  // namespace

extern "C" {

int os2ra_abi_version(void) { return OS2R_ES_ABI_VERSION; }

const char* os2ra_last_error(void) { return g_error.c_str(); }

int os2ra_es_perturb(const Os2rControlLayout* layout, int64_t npops, int32_t ndirs, uint32_t flags, uint64_t seed, uint32_t pop_offset,
                     uint32_t generation, const void* theta_dev, double nu, void* weights_dev, void* delta_dev, void* stream) {
  g_entry_point = "os2ra_es_perturb: ";
  if (const char* why = layout_refusal(layout)) return fail(OS2R_ERR_INVALID, why);
  if (const char* why = shape_refusal(layout, npops, ndirs, flags)) return fail(OS2R_ERR_INVALID, why);
  if (const int bad = scale_refusal(nu)) return fail(OS2R_ERR_INVALID, bad == 1 ? "nu must be finite" : "nu must be >= 0");
  if (!theta_dev) return fail(OS2R_ERR_INVALID, "null theta_dev");
  if (!weights_dev) return fail(OS2R_ERR_INVALID, "null weights_dev");
  const uintptr_t elem = layout->dtype == OS2R_F64 ? sizeof(double) : sizeof(float);
  if ((uintptr_t)theta_dev % (2 * elem)) return fail(OS2R_ERR_INVALID, "theta_dev must be aligned to a pair of its elements");
  if ((uintptr_t)weights_dev % (2 * elem)) return fail(OS2R_ERR_INVALID, "weights_dev must be aligned to a pair of its elements");
  if ((uintptr_t)delta_dev % (2 * elem)) return fail(OS2R_ERR_INVALID, "delta_dev must be aligned to a pair of its elements");
  {
    const uintptr_t M = (uintptr_t)npops, SM = (uintptr_t)ndirs * M, E = 2 * ((uintptr_t)layout->obs_dim + 1);
    const Span spans[] = {
        {"theta_dev", theta_dev, M * E * elem, false},
        {"weights_dev", weights_dev, 2 * SM * E * elem, true},
        {"delta_dev", delta_dev, SM * E * elem, true},
    };
    const std::string why = overlap_refusal(spans, sizeof(spans) / sizeof(spans[0]));
    if (!why.empty()) return fail(OS2R_ERR_INVALID, why);
  }
  // the device, from here on
  if (const int rc = check_device(layout->device)) return rc;
  DeviceGuard guard(layout->device);
  auto launch = [&](auto real) {
    using T = decltype(real);
    EsArgs<T> p;
    std::memset(&p, 0, sizeof(p));
    p.theta = (const T*)theta_dev; p.weights = (T*)weights_dev; p.delta = (T*)delta_dev;
    p.seed = seed; p.M = npops; p.pop_offset = pop_offset; p.generation = generation; p.S = ndirs; p.D = layout->obs_dim;
    p.nu = (T)nu;
    launch_es_perturb<T>(p, (hipStream_t)stream);
    return launched(0);
  };
  return layout->dtype == OS2R_F64 ? launch(double()) : launch(float());
}

int os2ra_es_update(const Os2rControlLayout* layout, int64_t npops, int32_t ndirs, int32_t top, uint32_t flags, uint64_t seed,
                    uint32_t pop_offset, uint32_t generation, const void* returns_dev, const void* theta_dev, double step_size,
                    double sigma_floor, void* theta_out_dev, void* sigma_r_dev, int32_t* count_dev, int32_t* used_dev, void* grad_dev,
                    int32_t* kept_dev, void* score_dev, void* stream) {
  g_entry_point = "os2ra_es_update: ";
  if (const char* why = layout_refusal(layout)) return fail(OS2R_ERR_INVALID, why);
  if (const char* why = shape_refusal(layout, npops, ndirs, flags)) return fail(OS2R_ERR_INVALID, why);
  if (top < 0) return fail(OS2R_ERR_INVALID, "top must be >= 0");
  if (const int bad = scale_refusal(step_size)) return fail(OS2R_ERR_INVALID, bad == 1 ? "step_size must be finite" : "step_size must be >= 0");
  if (const int bad = scale_refusal(sigma_floor)) return fail(OS2R_ERR_INVALID, bad == 1 ? "sigma_floor must be finite" : "sigma_floor must be >= 0");
  const bool select = top > 0 && top < ndirs;
  if (!returns_dev) return fail(OS2R_ERR_INVALID, "null returns_dev");
  if (!theta_dev) return fail(OS2R_ERR_INVALID, "null theta_dev");
  if (!theta_out_dev) return fail(OS2R_ERR_INVALID, "null theta_out_dev");
  if (!sigma_r_dev) return fail(OS2R_ERR_INVALID, "null sigma_r_dev");
  if (!count_dev) return fail(OS2R_ERR_INVALID, "null count_dev");
  if (!used_dev) return fail(OS2R_ERR_INVALID, "null used_dev");
  if (!kept_dev) return fail(OS2R_ERR_INVALID, "null kept_dev");
  if (select && !score_dev) return fail(OS2R_ERR_INVALID, "null score_dev with 0 < top < ndirs (the rank launch reads it)");
  const uintptr_t elem = layout->dtype == OS2R_F64 ? sizeof(double) : sizeof(float);
  if ((uintptr_t)theta_dev % (2 * elem)) return fail(OS2R_ERR_INVALID, "theta_dev must be aligned to a pair of its elements");
  if ((uintptr_t)theta_out_dev % (2 * elem)) return fail(OS2R_ERR_INVALID, "theta_out_dev must be aligned to a pair of its elements");
  if ((uintptr_t)grad_dev % (2 * elem)) return fail(OS2R_ERR_INVALID, "grad_dev must be aligned to a pair of its elements");
  if (select && (uintptr_t)score_dev % elem) return fail(OS2R_ERR_INVALID, "score_dev must be aligned to its elements");
  {
    const uintptr_t M = (uintptr_t)npops, SM = (uintptr_t)ndirs * M, E = 2 * ((uintptr_t)layout->obs_dim + 1);
    const Span spans[] = {
        {"returns_dev", returns_dev, 2 * SM * elem, false},
        {"theta_dev", theta_dev, M * E * elem, false},
        {"theta_out_dev", theta_out_dev, M * E * elem, true},
        {"sigma_r_dev", sigma_r_dev, M * elem, true},
        {"count_dev", count_dev, M * sizeof(int32_t), true},
        {"used_dev", used_dev, M * sizeof(int32_t), true},
        {"grad_dev", grad_dev, M * E * elem, true},
        {"kept_dev", kept_dev, SM * sizeof(int32_t), true},
        {"score_dev", select ? score_dev : nullptr, SM * elem, true},
    };
    const std::string why = overlap_refusal(spans, sizeof(spans) / sizeof(spans[0]));
    if (!why.empty()) return fail(OS2R_ERR_INVALID, why);
  }
  // the device, from here on
  if (const int rc = check_device(layout->device)) return rc;
  DeviceGuard guard(layout->device);
  auto launch = [&](auto real) {
    using T = decltype(real);
    EsArgs<T> p;
    std::memset(&p, 0, sizeof(p));
    p.returns = (const T*)returns_dev; p.theta = (const T*)theta_dev; p.theta_out = (T*)theta_out_dev; p.sigma_r = (T*)sigma_r_dev;
    p.count = count_dev; p.used = used_dev; p.grad = (T*)grad_dev; p.kept = kept_dev; p.score = select ? score_dev : nullptr;
    p.seed = seed; p.M = npops; p.pop_offset = pop_offset; p.generation = generation; p.S = ndirs; p.D = layout->obs_dim;
    p.top = top; p.select = select ? 1 : 0;
    p.step_size = (T)step_size; p.sigma_floor = (T)sigma_floor;
    launch_es_update<T>(p, (hipStream_t)stream);
    return launched(0);
  };
  return layout->dtype == OS2R_F64 ? launch(double()) : launch(float());
}

}  // extern "C"
