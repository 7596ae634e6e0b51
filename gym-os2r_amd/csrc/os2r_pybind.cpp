// os2r_pybind.cpp — thin pybind11 module over the C-ABI of include/os2r.h.
//
// One function per entry point, integer addresses in (tensor.data_ptr(), ctypes.addressof of
// the config struct, the raw hipStream_t), status codes out; no torch types, no logic.  The GIL is
// released around every call.  gym_os2r_amd.sim uses it when OS2R_BINDING=pybind11 (default: ctypes).
// An entry point is bound by its prototype (`bind`): a binding that disagrees with the header does not compile.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/os2r.h"
#include "../../include/os2r_record.h"

namespace py = pybind11;
using addr = std::uintptr_t;

static Os2rSim* H(addr h) { return reinterpret_cast<Os2rSim*>(h); }
static void* P(addr a) { return reinterpret_cast<void*>(a); }

// A parameter of the C-ABI as Python passes it: a pointer as an integer address, cast back to its own type; anything else as it is.
template <typename T> struct Arg { using py_type = T; static T to_c(T v) { return v; } };
template <typename T> struct Arg<T*> { using py_type = addr; static T* to_c(addr a) { return reinterpret_cast<T*>(a); } };

// One entry point under `name`, its Python signature derived from the C prototype.
template <typename... A>
static void bind(py::module_& m, const char* name, int (*fn)(A...)) {
  m.def(name, [fn](typename Arg<A>::py_type... a) { return fn(Arg<A>::to_c(a)...); }, py::call_guard<py::gil_scoped_release>());
}

PYBIND11_MODULE(_os2r_py, m) {
  m.doc() = "pybind11 binding of libos2r.so (MI355X batched monopod stepper)";
  bind(m, "destroy", &os2r_destroy);
  bind(m, "reset", &os2r_reset);
  bind(m, "step", &os2r_step);
  bind(m, "rollout", &os2r_rollout);
  bind(m, "rollout_policy", &os2r_rollout_policy);
  bind(m, "rollout_policy_noisy", &os2r_rollout_policy_noisy);
  bind(m, "rollout_policy_scheduled", &os2r_rollout_policy_scheduled);
  bind(m, "model_is_compiled_in", &os2r_model_is_compiled_in);
  bind(m, "get_action_violations", &os2r_get_action_violations);
  bind(m, "get_state", &os2r_get_state);
  bind(m, "set_state", &os2r_set_state);
  bind(m, "get_solver_state", &os2r_get_solver_state);
  bind(m, "set_solver_state", &os2r_set_solver_state);
  bind(m, "get_action_history", &os2r_get_action_history);
  bind(m, "set_action_history", &os2r_set_action_history);
  bind(m, "set_params", &os2r_set_params);
  bind(m, "get_params", &os2r_get_params);
  bind(m, "get_episode_info", &os2r_get_episode_info);
  bind(m, "set_episode_info", &os2r_set_episode_info);
  bind(m, "copy_envs", &os2r_copy_envs);
  bind(m, "lqr_gains", &os2r_lqr_gains);
  bind(m, "set_step_count", &os2r_set_step_count);
  bind(m, "set_work_counters", &os2r_set_work_counters);
  bind(m, "set_done_reasons", &os2r_set_done_reasons);
  bind(m, "set_done_mask", &os2r_set_done_mask);

  // the calls whose Python shape is not the C one: values come back in a tuple, eps is three doubles, the path a str
  m.def("abi_version", &os2r_abi_version);
  m.def("abi_minor", &os2r_abi_minor);
  m.def("create", [](addr cfg) {
    Os2rSim* s = nullptr;
    int rc;
    { py::gil_scoped_release rel; rc = os2r_create(reinterpret_cast<const Os2rConfig*>(cfg), &s); }
    return py::make_tuple(rc, reinterpret_cast<addr>(s));
  });
  m.def("linearize", [](addr h, addr act, double eq, double ev, double ea, addr next, addr ja, addr jb, addr st) {
    const double eps[3] = {eq, ev, ea};
    return os2r_linearize(H(h), P(act), eps, P(next), P(ja), P(jb), P(st)); }, py::call_guard<py::gil_scoped_release>());
  m.def("get_step_count", [](addr h) { uint64_t v = 0; int rc = os2r_get_step_count(H(h), &v); return py::make_tuple(rc, v); });
  m.def("bench_steps", [](addr h, int n, addr st) {
    float ms = 0.f;
    int rc;
    { py::gil_scoped_release rel; rc = os2r_bench_steps(H(h), n, P(st), &ms); }
    return py::make_tuple(rc, ms);
  });
  m.def("bench_enqueue", [](addr h, int n, addr st) {
    py::gil_scoped_release rel;
    return os2r_bench_steps(H(h), n, P(st), nullptr);
  });
  m.def("bench_steps_multi", [](std::vector<addr> hs, std::vector<addr> sts, int n) {
    std::vector<Os2rSim*> sims; std::vector<void*> streams;
    for (addr h : hs) sims.push_back(H(h));
    for (addr s : sts) streams.push_back(P(s));
    if (sims.size() != streams.size()) return (int)OS2R_ERR_INVALID;
    py::gil_scoped_release rel;
    return os2r_bench_steps_multi(sims.data(), streams.data(), (int)sims.size(), n);
  });
  m.def("get_violation_mirror", [](addr h) { const volatile uint32_t* w = nullptr; int rc = os2r_get_violation_mirror(H(h), &w); return py::make_tuple(rc, (addr)w); });
  m.def("register_model_kernels", [](addr model, int dtype, int device, const std::string& path) {
    return os2r_register_model_kernels((const Os2rModel*)P(model), dtype, device, path.c_str()); });
  // libos2r_record.so (include/os2r_record.h)
  bind(m, "rollout_policy_recorded", &os2rr_rollout_policy_recorded);
  m.def("record_last_error", []() { return std::string(os2rr_last_error()); });
  m.def("last_error", [](addr h) { return std::string(os2r_last_error(H(h))); });
}
