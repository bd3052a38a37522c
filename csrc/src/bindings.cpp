// Python bindings (pybind11) of the native engine: gol_amd._gol.
//
// Python only orchestrates (process-group bootstrap, tensors, tests, bench);
// the generation loop, kernels, halo schedule, I/O and termination logic are
// native.  Long-running calls release the GIL so in-process ranks can run
// on Python threads.
#include <pybind11/functional.h>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>
#include <optional>
#include <thread>
#include <tuple>

#include "gol/backend.hpp"
#include "gol/batch.hpp"
#include "gol/cpu_ref.hpp"
#include "gol/decomp.hpp"
#include "gol/engine.hpp"
#include "gol/fingerprint.hpp"
#include "gol/io.hpp"
#include "gol/numa.hpp"
#include "gol/transport.hpp"

namespace py = pybind11;
using namespace gol;

namespace {

// torch.distributed (or anything else) implemented in Python.  Buffers are
// passed as (address, nbytes) pairs in the backend's address space.
class CallbackTransport final : public Transport {
 public:
  using ExchangeFn = std::function<void(py::list, std::uintptr_t)>;
  using ReduceFn = std::function<void(std::uintptr_t, size_t, std::uintptr_t)>;
  using BarrierFn = std::function<void()>;
  CallbackTransport(int rank, int size, ExchangeFn ex, ReduceFn red, BarrierFn bar, ReduceFn sum)
      : rank_(rank), size_(size), ex_(std::move(ex)), red_(std::move(red)), bar_(std::move(bar)),
        sum_(std::move(sum)) {}
  int rank() const override { return rank_; }
  int size() const override { return size_; }
  const char* name() const override { return "callback"; }
  void exchange(const std::vector<P2POp>& ops, void* stream) override {
    py::gil_scoped_acquire gil;
    py::list l;
    for (const auto& op : ops)
      l.append(py::make_tuple(op.send, op.peer, reinterpret_cast<std::uintptr_t>(op.buf), op.bytes));
    ex_(l, reinterpret_cast<std::uintptr_t>(stream));
  }
  void allreduce_max_u32(uint32_t* buf, size_t n, void* stream) override {
    py::gil_scoped_acquire gil;
    red_(reinterpret_cast<std::uintptr_t>(buf), n, reinterpret_cast<std::uintptr_t>(stream));
  }
  void allreduce_sum_u64(uint64_t* buf, size_t n, void* stream) override {
    GOL_REQUIRE(bool(sum_), "callback transport: no sum callback (census needs one)");
    py::gil_scoped_acquire gil;
    sum_(reinterpret_cast<std::uintptr_t>(buf), n, reinterpret_cast<std::uintptr_t>(stream));
  }
  void barrier() override {
    py::gil_scoped_acquire gil;
    bar_();
  }

 private:
  int rank_, size_;
  ExchangeFn ex_;
  ReduceFn red_;
  BarrierFn bar_;
  ReduceFn sum_;  // SUM of n 64-bit counts (may be empty: a transport built without it)
};

py::array_t<uint8_t> to_array(std::vector<uint8_t>&& v, int64_t rows, int64_t cols) {
  auto* heap = new std::vector<uint8_t>(std::move(v));
  py::capsule owner(heap, [](void* p) { delete static_cast<std::vector<uint8_t>*>(p); });
  return py::array_t<uint8_t>({rows, cols}, {cols, int64_t(1)}, heap->data(), owner);
}

const uint8_t* grid_ptr(const py::array_t<uint8_t, py::array::c_style | py::array::forcecast>& a,
                        int64_t rows, int64_t cols) {
  GOL_REQUIRE(a.ndim() == 2 && a.shape(0) == rows && a.shape(1) == cols,
              "expected a " + std::to_string(rows) + "x" + std::to_string(cols) + " uint8 array");
  return a.data();
}

// Whether the backend runs the combination (Backend::refusal() is empty).
bool runs(const Backend& b, Layout l, const std::string& rule, const std::string& boundary, bool census = false,
          bool fingerprint = false) {
  const Boundary bd = parse_boundary(boundary);
  return b.refusal(l, parse_rule(rule), bd, {bd == Boundary::Dead, census, fingerprint}).empty();
}

}  // namespace

// ClusterCensus as NumPy arrays: (clusters, universe, signature, cells, height, width, spanning, ms, count_ms).
template <class T>
py::array_t<T> copy_array(const std::vector<T>& v) {
  py::array_t<T> a(static_cast<py::ssize_t>(v.size()));
  std::copy(v.begin(), v.end(), a.mutable_data());
  return a;
}
py::tuple census_arrays(const ClusterCensus& c) {
  return py::make_tuple(copy_array(c.clusters), copy_array(c.universe), copy_array(c.signature), copy_array(c.cells),
                        copy_array(c.height), copy_array(c.width), copy_array(c.spanning), c.ms, c.count_ms);
}

PYBIND11_MODULE(_gol, m) {
  m.doc() = "gol-mi355x native engine (CDNA4 HIP kernels, RCCL halos, C++ runtime)";
  py::register_exception<Error>(m, "GolError", PyExc_RuntimeError);

  py::enum_<Layout>(m, "Layout").value("U8", Layout::U8).value("Bits", Layout::Bits);

  py::class_<Extent>(m, "Extent")
      .def_readonly("begin", &Extent::begin)
      .def_readonly("end", &Extent::end)
      .def("size", &Extent::size)
      .def("__repr__", [](const Extent& e) {
        return "Extent(" + std::to_string(e.begin) + ", " + std::to_string(e.end) + ")";
      });

  py::class_<Decomposition>(m, "Decomposition")
      .def(py::init<int64_t, int64_t, int, int, int64_t>(), py::arg("W"), py::arg("H"), py::arg("Px"),
           py::arg("Py"), py::arg("col_unit") = 1)
      .def_static("make", &Decomposition::make, py::arg("W"), py::arg("H"), py::arg("nranks"),
                  py::arg("spec") = "auto", py::arg("col_unit") = 1)
      .def_readonly("W", &Decomposition::W)
      .def_readonly("H", &Decomposition::H)
      .def_readonly("Px", &Decomposition::Px)
      .def_readonly("Py", &Decomposition::Py)
      .def("nranks", &Decomposition::nranks)
      .def("rows", &Decomposition::rows)
      .def("cols", &Decomposition::cols)
      .def("px_of", &Decomposition::px_of)
      .def("py_of", &Decomposition::py_of)
      .def("rank_of", &Decomposition::rank_of)
      .def("neighbors", [](const Decomposition& d, int rank, bool plane) { return d.neighbors(rank, plane); },
           py::arg("rank"), py::arg("plane") = false)
      .def("describe", &Decomposition::describe);
  m.def("split_range", &split_range);

  py::class_<TileGeom>(m, "TileGeom")
      .def_static("make", &TileGeom::make)
      .def_readonly("H", &TileGeom::H)
      .def_readonly("W", &TileGeom::W)
      .def_readonly("Dv", &TileGeom::Dv)
      .def_readonly("hw", &TileGeom::hw)
      .def_readonly("pitch", &TileGeom::pitch)
      .def("R", &TileGeom::R)
      .def("Wc", &TileGeom::Wc)
      .def("Wp", &TileGeom::Wp)
      .def("bytes", &TileGeom::bytes);

  // Runtime tuning (gol/tuning.hpp).  Python passes a dict: LifeConfig.tune,
  // make_backend(tune=...), bench.py / gol_amd.cli --tune key=value.
  py::class_<Tuning>(m, "Tuning")
      .def(py::init<>())
      .def_static("from_env", &Tuning::from_env)
      .def("set", py::overload_cast<const std::string&, const std::string&>(&Tuning::set),
           py::return_value_policy::reference_internal)
      .def("get", &Tuning::s)
      .def("is_default", &Tuning::is_default)
      .def("source", &Tuning::source)
      .def("values", &Tuning::values)
      .def("changed", &Tuning::changed)
      .def("summary", &Tuning::summary)
      .def("copy", [](const Tuning& t) { return Tuning(t); });
  m.def("tuning_keys", []() {
    py::list out;
    for (const TuningKey& k : tuning_keys()) {
      py::dict d;
      d["key"] = k.key;
      d["env"] = k.env;
      d["default"] = k.dflt;
      d["type"] = std::string(1, k.type);
      d["class"] = k.cls;
      d["doc"] = k.doc;
      out.append(d);
    }
    return out;
  });

  py::class_<Backend, std::shared_ptr<Backend>>(m, "Backend")
      .def("name", &Backend::name)
      .def("launch_paths", &Backend::launch_paths)
      .def("tuning", &Backend::tuning, py::return_value_policy::copy)
      .def("is_device", &Backend::is_device)
      .def("device", &Backend::device)
      .def("stream", [](const Backend& b) { return reinterpret_cast<std::uintptr_t>(b.stream()); })
      .def("synchronize", &Backend::synchronize, py::call_guard<py::gil_scoped_release>())
      // Backend::refusal() by the question asked: the named feature with
      // what else the arguments give; a "dead" boundary implies the plane.
      .def("supports_rule", [](const Backend& b, Layout l, const std::string& rule) { return runs(b, l, rule, "torus"); })
      .def("supports_boundary", [](const Backend& b, Layout l, const std::string& rule, const std::string& boundary) {
        return runs(b, l, rule, boundary) || boundary == "torus";  // whether it runs the rule: supports_rule
      })
      .def("supports_census", [](const Backend& b, Layout l, const std::string& rule, const std::string& boundary) {
        return runs(b, l, rule, boundary, true);
      })
      .def("supports_fingerprint",
           [](const Backend& b, Layout l, const std::string& rule, const std::string& boundary, bool census) {
             return runs(b, l, rule, boundary, census, true);
           },
           py::arg("layout"), py::arg("rule"), py::arg("boundary"), py::arg("census") = false)
      .def("plane_kernel", [](const Backend& b, Layout l) { return b.feature_kernel(l, BlockMode::Plane); })
      .def("census_kernel", [](const Backend& b, Layout l) { return b.feature_kernel(l, BlockMode::Census); })
      .def("fingerprint_kernel", [](const Backend& b, Layout l) { return b.feature_kernel(l, BlockMode::Fingerprint); })
      .def("bind_thread", &Backend::bind_thread);
  m.def("cpu_backend",
        [](int threads, int drift, std::optional<Tuning> tune) {
          return std::shared_ptr<Backend>(make_cpu_backend(threads, drift, tune ? *tune : Tuning::from_env()));
        },
        py::arg("threads") = 0, py::arg("drift") = -1, py::arg("tune") = py::none());
  m.def("hip_backend",
        [](int device, std::optional<Tuning> tune) {
          return std::shared_ptr<Backend>(make_hip_backend(device, tune ? *tune : Tuning::from_env()));
        },
        py::arg("device") = 0, py::arg("tune") = py::none());
  m.def("hip_available", &hip_available);
  // The HIP engine's refusal of a combination ("": it runs), without a device.
  m.def("hip_refusal",
        [](Layout l, const std::string& rule, const std::string& boundary, bool census, bool fingerprint, bool u8_lds) {
          const Boundary b = parse_boundary(boundary);
          return hip_refusal(l, parse_rule(rule), b, {b == Boundary::Dead, census, fingerprint}, u8_lds);
        },
        py::arg("layout"), py::arg("rule"), py::arg("boundary") = "torus", py::arg("census") = false,
        py::arg("fingerprint") = false, py::arg("u8_lds") = false);
  // Life-like rules (common.hpp): canonical text of a rule given by name or in
  // B/S notation, the named rules, and the rules compiled for the HIP engine.
  m.def("parse_rule", [](const std::string& s) { return rule_string(parse_rule(s)); });
  m.def("rule_names", []() {
    py::dict d;
    for (const RuleName& n : kRuleNames) d[n.name] = rule_string(n.rule);
    return d;
  });
  m.def("hip_rules", []() {
    std::vector<std::string> v{rule_string(Rule{})};
    for (const Rule r : hip_rules()) v.push_back(rule_string(r));
    return v;
  });
  m.def("hip_pci_bus_id", &hip_pci_bus_id);
  m.def("hip_release_errors", &hip_release_errors);
  m.def("hip_uuid", &hip_uuid);
  m.def("parse_cpulist", &parse_cpulist);
  m.def("pci_numa_node", &pci_numa_node);
  m.def("pinned_numa_node", &pinned_numa_node);

  py::class_<Transport, std::shared_ptr<Transport>>(m, "Transport")
      .def("rank", &Transport::rank)
      .def("size", &Transport::size)
      .def("name", &Transport::name)
      .def("comm_count", &Transport::comm_count)
      .def("comm_device", &Transport::comm_device)
      .def("barrier", &Transport::barrier, py::call_guard<py::gil_scoped_release>())
      // Raw access for plumbing tests: ops = [(send, peer, address, bytes)],
      // addresses in the transport's address space (device memory for rccl).
      .def("exchange",
           [](Transport& t, const std::vector<std::tuple<bool, int, std::uintptr_t, size_t>>& ops,
              std::uintptr_t stream) {
             std::vector<P2POp> v;
             for (const auto& [send, peer, addr, bytes] : ops)
               v.push_back({send, peer, reinterpret_cast<void*>(addr), bytes});
             py::gil_scoped_release rel;
             t.exchange(v, reinterpret_cast<void*>(stream));
           })
      .def("allreduce_max_u32",
           [](Transport& t, std::uintptr_t addr, size_t n, std::uintptr_t stream) {
             py::gil_scoped_release rel;
             t.allreduce_max_u32(reinterpret_cast<uint32_t*>(addr), n, reinterpret_cast<void*>(stream));
           })
      .def("allreduce_sum_u64",
           [](Transport& t, std::uintptr_t addr, size_t n, std::uintptr_t stream) {
             py::gil_scoped_release rel;
             t.allreduce_sum_u64(reinterpret_cast<uint64_t*>(addr), n, reinterpret_cast<void*>(stream));
           });
  m.def("self_transport", []() { return std::shared_ptr<Transport>(new SelfTransport()); });
  py::class_<ThreadHub, std::shared_ptr<ThreadHub>>(m, "ThreadHub").def(py::init<int>());
  m.def("thread_transport",
        [](std::shared_ptr<ThreadHub> hub, int rank, std::shared_ptr<Backend> be, std::optional<Tuning> tune) {
          return std::shared_ptr<Transport>(
              new ThreadTransport(std::move(hub), rank, be.get(), tune ? *tune : Tuning::from_env()));
        },
        py::arg("hub"), py::arg("rank"), py::arg("backend"), py::arg("tune") = py::none(), py::keep_alive<0, 3>());
  m.def("callback_transport",
        [](int rank, int size, CallbackTransport::ExchangeFn ex, CallbackTransport::ReduceFn red,
           CallbackTransport::BarrierFn bar, CallbackTransport::ReduceFn sum) {
          return std::shared_ptr<Transport>(new CallbackTransport(rank, size, ex, red, bar, sum));
        },
        py::arg("rank"), py::arg("size"), py::arg("exchange"), py::arg("allreduce_max_u32"), py::arg("barrier"),
        py::arg("allreduce_sum_u64") = CallbackTransport::ReduceFn());
  m.def("rccl_unique_id", []() {
    auto v = rccl_unique_id();
    return py::bytes(reinterpret_cast<const char*>(v.data()), v.size());
  });
  m.def("rccl_transport",
        [](py::bytes uid, int rank, int nranks, int device, std::optional<Tuning> tune) {
          std::string s = uid;
          std::vector<uint8_t> v(s.begin(), s.end());
          const Tuning t = tune ? *tune : Tuning::from_env();
          std::shared_ptr<Transport> tr;
          {
            py::gil_scoped_release rel;
            tr = make_rccl_transport(v, rank, nranks, device, t);
          }
          return tr;
        },
        py::arg("uid"), py::arg("rank"), py::arg("nranks"), py::arg("device"), py::arg("tune") = py::none());

  py::class_<EngineConfig>(m, "EngineConfig")
      .def(py::init<>())
      .def_readwrite("W", &EngineConfig::W)
      .def_readwrite("H", &EngineConfig::H)
      .def_readwrite("layout", &EngineConfig::layout)
      .def_property("rule", [](const EngineConfig& c) { return rule_string(c.rule); },
                    [](EngineConfig& c, const std::string& s) { c.rule = parse_rule(s); })
      .def_property("boundary", [](const EngineConfig& c) { return std::string(boundary_name(c.boundary)); },
                    [](EngineConfig& c, const std::string& s) { c.boundary = parse_boundary(s); })
      .def_readwrite("census", &EngineConfig::census)
      .def_readwrite("fingerprint", &EngineConfig::fingerprint)
      .def_readwrite("decomp", &EngineConfig::decomp)
      .def_readwrite("gen_limit", &EngineConfig::gen_limit)
      .def_readwrite("check_similarity", &EngineConfig::check_similarity)
      .def_readwrite("sim_freq", &EngineConfig::sim_freq)
      .def_readwrite("start_gen", &EngineConfig::start_gen)
      .def_readwrite("sim_phase", &EngineConfig::sim_phase)
      .def_readwrite("tmax", &EngineConfig::tmax)
      .def_readwrite("epoch", &EngineConfig::epoch)
      .def_readwrite("poll_gens", &EngineConfig::poll_gens)
      .def_readwrite("overlap", &EngineConfig::overlap)
      .def_readwrite("lagged_poll", &EngineConfig::lagged_poll)
      .def_readwrite("timing_barriers", &EngineConfig::timing_barriers)
      .def_readwrite("self_exchange", &EngineConfig::self_exchange)
      .def_readwrite("u8_compute", &EngineConfig::u8_compute)
      .def_readwrite("graphs", &EngineConfig::graphs)
      .def_readwrite("watchdog_s", &EngineConfig::watchdog_s)
      .def_readwrite("tune", &EngineConfig::tune);

  py::class_<RunResult>(m, "RunResult")
      .def_readonly("generations", &RunResult::generations)
      .def_readonly("executed", &RunResult::executed)
      .def_readonly("first_unchanged", &RunResult::first_unchanged)
      .def_readonly("extinct", &RunResult::extinct)
      .def_readonly("stop_reason", &RunResult::stop_reason)
      .def_readonly("loop_ms", &RunResult::loop_ms)
      .def_readonly("exchanges", &RunResult::exchanges)
      .def_readonly("polls", &RunResult::polls)
      .def_readonly("kernel_launches", &RunResult::kernel_launches)
      .def_readonly("overlapped", &RunResult::overlapped)
      .def_readonly("graph_launches", &RunResult::graph_launches)
      .def_readonly("halo_bytes", &RunResult::halo_bytes)
      .def_readonly("linked_launches", &RunResult::linked_launches)
      .def_readonly("phase_timed", &RunResult::phase_timed)
      .def_readonly("compute_ms", &RunResult::compute_ms)
      .def_readonly("halo_ms", &RunResult::halo_ms)
      .def_readonly("fill_ms", &RunResult::fill_ms)
      .def_readonly("allreduce_ms", &RunResult::allreduce_ms)
      .def_property_readonly("population", [](const RunResult& r) {
        py::array_t<int64_t> a(static_cast<py::ssize_t>(r.population.size()));
        std::copy(r.population.begin(), r.population.end(), a.mutable_data());
        return a;
      })
      .def_property_readonly("fingerprint", [](const RunResult& r) {
        py::array_t<uint64_t> a(static_cast<py::ssize_t>(r.fingerprint.size()));
        std::copy(r.fingerprint.begin(), r.fingerprint.end(), a.mutable_data());
        return a;
      });
  py::class_<CycleResult>(m, "CycleResult")
      .def_readonly("period", &CycleResult::period)
      .def_readonly("generation", &CycleResult::generation)
      .def_readonly("repeats_from", &CycleResult::repeats_from)
      .def_readonly("confirmations", &CycleResult::confirmations)
      .def_readonly("false_candidates", &CycleResult::false_candidates)
      .def_readonly("stop_reason", &CycleResult::stop_reason)
      .def_readonly("loop_ms", &CycleResult::loop_ms)
      .def_property_readonly("fingerprint", [](const CycleResult& r) {
        py::array_t<uint64_t> a(static_cast<py::ssize_t>(r.fingerprint.size()));
        std::copy(r.fingerprint.begin(), r.fingerprint.end(), a.mutable_data());
        return a;
      });

  py::class_<Engine>(m, "Engine")
      .def(py::init([](const EngineConfig& c, std::shared_ptr<Backend> be, std::shared_ptr<Transport> tr) {
             return new Engine(c, be.get(), tr.get());
           }),
           py::keep_alive<1, 3>(), py::keep_alive<1, 4>())
      .def_property_readonly("config", &Engine::config, py::return_value_policy::copy)
      .def_property_readonly("rank", &Engine::rank)
      .def_property_readonly("rows", &Engine::rows)
      .def_property_readonly("cols", &Engine::cols)
      .def_property_readonly("decomp", &Engine::decomp)
      .def_property_readonly("geom", &Engine::geom)
      .def_property_readonly("compute_geom", &Engine::compute_geom)
      .def_property_readonly("epoch_depth", &Engine::epoch_depth)
      .def_property_readonly("tmax", &Engine::tmax)
      .def("overlap", &Engine::overlap)
      .def("overlap_mode", &Engine::overlap_mode)
      .def_property_readonly("trial_ms_plain", &Engine::trial_ms_plain)
      .def_property_readonly("trial_ms_trigger", &Engine::trial_ms_trigger)
      .def("poll_mode", &Engine::poll_mode)
      .def_property_readonly("poll_trial_ms_joined", &Engine::poll_trial_ms_joined)
      .def_property_readonly("poll_trial_ms_side", &Engine::poll_trial_ms_side)
      .def_property_readonly("poll_trial_ms_side_steady", &Engine::poll_trial_ms_side_steady)
      .def("triggered_sends", &Engine::triggered_sends)
      .def("quiet_mode", &Engine::quiet_mode)
      .def_property_readonly("quiet_blocks_dense", &Engine::quiet_blocks_dense)
      .def_property_readonly("quiet_blocks_scout", &Engine::quiet_blocks_scout)
      .def_property_readonly("quiet_blocks_skip", &Engine::quiet_blocks_skip)
      .def_property_readonly("quiet_waves_launched", &Engine::quiet_waves_launched)
      .def_property_readonly("quiet_waves_skipped", &Engine::quiet_waves_skipped)
      .def_property_readonly("quiet_list", &Engine::quiet_list)
      .def_property_readonly("quiet_candidates", &Engine::quiet_candidates)
      .def_property_readonly("quiet_cols", &Engine::quiet_cols)
      .def("quiet_cols_counts", &Engine::quiet_cols_counts)
      .def_property_readonly("spine_generation", &Engine::spine_generation)
      .def_property_readonly("tail_overshoots", &Engine::tail_overshoots)
      .def_property_readonly("tail_replays", &Engine::tail_replays)
      .def_property("phase_timing", &Engine::phase_timing, &Engine::set_phase_timing)
      .def("graphs", &Engine::graphs)
      .def_property("generation", &Engine::generation, &Engine::set_generation)
      .def_property_readonly("drift", &Engine::drift)
      .def_property_readonly("drifting", &Engine::drifting)
      .def_property_readonly("row_ring", &Engine::row_ring)
      .def_property_readonly("row_ring_fallback", &Engine::row_ring_fallback)
      .def_property_readonly("via_bits", &Engine::via_bits)
      .def("normalize", &Engine::normalize, py::call_guard<py::gil_scoped_release>())
      .def("current_buffer", [](Engine& e) { return reinterpret_cast<std::uintptr_t>(e.current_buffer()); })
      .def("load_cells",
           [](Engine& e, py::array_t<uint8_t, py::array::c_style | py::array::forcecast> a) {
             const uint8_t* p = grid_ptr(a, e.rows().size(), e.cols().size());
             py::gil_scoped_release rel;
             e.load_cells(p, e.cols().size());
           })
      .def("load_global",
           [](Engine& e, py::array_t<uint8_t, py::array::c_style | py::array::forcecast> a) {
             const uint8_t* p = grid_ptr(a, e.decomp().H, e.decomp().W);
             py::gil_scoped_release rel;
             e.load_global(p, e.decomp().W);
           })
      .def("store_cells",
           [](Engine& e, bool ascii) {
             std::vector<uint8_t> v(size_t(e.rows().size() * e.cols().size()));
             {
               py::gil_scoped_release rel;
               e.store_cells(v.data(), e.cols().size(), ascii);
             }
             return to_array(std::move(v), e.rows().size(), e.cols().size());
           },
           py::arg("ascii") = false)
      // Owned rows [r0, r0 + n) only (a band of a grid too large for a host copy).
      .def("store_rows",
           [](Engine& e, int64_t r0, int64_t n, bool ascii) {
             std::vector<uint8_t> v(size_t(std::max<int64_t>(0, n) * e.cols().size()));
             {
               py::gil_scoped_release rel;
               e.store_rows(v.data(), e.cols().size(), r0, n, ascii);
             }
             return to_array(std::move(v), n, e.cols().size());
           },
           py::arg("r0"), py::arg("n"), py::arg("ascii") = false)
      .def("init_random", &Engine::init_random, py::arg("seed"), py::arg("density") = 0.5,
           py::call_guard<py::gil_scoped_release>())
      .def("alive_count", &Engine::alive_count, py::call_guard<py::gil_scoped_release>())
      .def("fingerprint", &Engine::fingerprint, py::call_guard<py::gil_scoped_release>())
      // Views (Engine::density / store_window / place): global coordinates,
      // every rank calls them.
      .def("density",
           [](Engine& e, int64_t bx, int64_t by) {
             GOL_REQUIRE(bx >= 1 && by >= 1, "density: block sizes must be at least 1");
             const int64_t nby = ceil_div(e.decomp().H, by), nbx = ceil_div(e.decomp().W, bx);
             const bool fits = nbx <= Backend::kDensityBlocksMax && nby <= Backend::kDensityBlocksMax &&
                               nbx * nby <= Backend::kDensityBlocksMax;
             py::array_t<int64_t> a({fits ? nby : 0, fits ? nbx : 0});  // the engine refuses the rest by name
             auto* out = reinterpret_cast<uint64_t*>(a.mutable_data());
             {
               py::gil_scoped_release rel;
               e.density(bx, by, out);
             }
             return a;
           },
           py::arg("bx"), py::arg("by"))
      .def("store_window",
           [](Engine& e, int64_t x, int64_t y, int64_t w, int64_t h, bool ascii) {
             // The engine checks the rectangle before it touches the array.
             const bool fits = w >= 1 && h >= 1 && w <= Backend::kWindowCellsMax / h;
             std::vector<uint8_t> v(fits ? size_t(w * h) : 0);
             {
               py::gil_scoped_release rel;
               e.store_window(x, y, w, h, v.data(), ascii);
             }
             return to_array(std::move(v), h, w);
           },
           py::arg("x"), py::arg("y"), py::arg("w"), py::arg("h"), py::arg("ascii") = false)
      .def("place",
           [](Engine& e, py::array_t<uint8_t, py::array::c_style | py::array::forcecast> a, int64_t x, int64_t y,
              const std::string& mode) {
             GOL_REQUIRE(a.ndim() == 2, "place: expected a 2-D array of cells");
             GOL_REQUIRE(mode == "copy" || mode == "or", "place: mode '" + mode + "' (want copy or or)");
             const int64_t h = a.shape(0), w = a.shape(1);
             const uint8_t* p = a.data();
             py::gil_scoped_release rel;
             e.place(x, y, w, h, p, mode == "or" ? Backend::kPlaceOr : Backend::kPlaceCopy);
           },
           py::arg("cells"), py::arg("x"), py::arg("y"), py::arg("mode") = "copy")
      .def("find_cycle", &Engine::find_cycle, py::arg("max_gens"), py::arg("max_period") = 64, py::arg("chunk") = 0,
           py::call_guard<py::gil_scoped_release>())
      .def("run", &Engine::run, py::call_guard<py::gil_scoped_release>())
      .def("advance", &Engine::advance, py::call_guard<py::gil_scoped_release>())
      .def("run_until", &Engine::run_until, py::call_guard<py::gil_scoped_release>())
      .def("halo_exchange", &Engine::halo_exchange, py::call_guard<py::gil_scoped_release>())
      .def("step_block", &Engine::step_block, py::call_guard<py::gil_scoped_release>())
      .def("read_text", [](Engine& e, const std::string& path) {
        std::vector<uint8_t> tile;
        {
          py::gil_scoped_release rel;
          read_text_tile(path, e.decomp().W, e.decomp().H, e.rows(), e.cols(), tile);
          e.load_cells(tile.data(), e.cols().size());
        }
      })
      .def("write_text", [](Engine& e, const std::string& path, bool create) {
        std::vector<uint8_t> tile(size_t(e.rows().size() * e.cols().size()));
        py::gil_scoped_release rel;
        e.store_cells(tile.data(), e.cols().size(), false);
        if (create) create_text_file(path, e.decomp().W, e.decomp().H);
        write_text_tile(path, e.decomp().W, e.decomp().H, e.rows(), e.cols(), tile.data(), e.cols().size());
      }, py::arg("path"), py::arg("create") = true);

  // ---- quiet-tile skipping: the pure decision logic (gol/quiet.hpp) ----
  m.attr("QUIET_DIRTY") = quiet::kDirty;
  m.attr("QUIET_TOP") = quiet::kTop;
  m.attr("QUIET_BOT") = quiet::kBot;
  m.attr("QUIET_LEFT") = quiet::kLeft;
  m.attr("QUIET_RIGHT") = quiet::kRight;
  m.def("quiet_may_skip", [](const std::vector<uint32_t>& nb) {
    GOL_REQUIRE(nb.size() == 9, "quiet_may_skip: nine tile words (3 x 3, row-major)");
    return quiet::may_skip(nb.data());
  });
  m.def("quiet_neighbour", &quiet::neighbour, py::arg("kcol"), py::arg("grp"), py::arg("i"), py::arg("ncolw"),
        py::arg("nseg"));
  m.def("quiet_marks_neighbours", &quiet::marks_neighbours);
  m.def("quiet_flag_words", [](int T) { return quiet::flag_words(T); });
  m.def("quiet_flag_delta", [](uint32_t old_word, uint32_t new_word, int w) {
    return (unsigned long long)quiet::flag_delta(old_word, new_word, w);
  });
  m.def("quiet_flag_levels", [](unsigned long long count, int w) { return quiet::flag_levels(count, w); });
  py::class_<quiet::ListModel>(m, "QuietListModel")
      .def(py::init<int, int, int>(), py::arg("ncolw"), py::arg("nseg"), py::arg("T"))
      .def("block", &quiet::ListModel::block, py::arg("fresh"), py::arg("follow"))
      .def("words", &quiet::ListModel::words)
      .def("words_before", &quiet::ListModel::words_before)
      .def("launched", &quiet::ListModel::launched)
      .def("candidates", &quiet::ListModel::candidates)
      .def("flags", &quiet::ListModel::flags)
      .def("flag_counts", &quiet::ListModel::flag_counts);
  // The column records (tuning quiet_cols).
  m.attr("QUIET_COLS") = quiet::kCols;
  m.attr("QUIET_COL_LANES") = quiet::kColLanes;
  m.def("quiet_col_standin", &quiet::col_standin);
  m.def("quiet_col_source", &quiet::col_source, py::arg("above"), py::arg("same"), py::arg("below"));
  m.def("quiet_window_spread", [](unsigned long long src, int own) { return (unsigned long long)quiet::window_spread(src, own); });
  m.def("quiet_window_groups", [](unsigned long long win, int own, int g) { return quiet::window_groups(win, own, g); });
  m.def("quiet_group_columns",
        [](uint32_t hit, int own, int g) { return (unsigned long long)quiet::group_columns(hit, own, g); });
  // rec[i]: the records of tile i of the neighbourhood (empty: none valid), words[i] its word.
  m.def("quiet_window",
        [](const std::vector<std::vector<uint32_t>>& rec, const std::vector<uint32_t>& words, int own_l, int own, int own_r) {
          GOL_REQUIRE(rec.size() == 9 && words.size() == 9, "quiet_window: nine tiles (3 x 3, row-major)");
          const uint32_t* r[9];
          for (int i = 0; i < 9; ++i) {
            GOL_REQUIRE(rec[i].empty() || rec[i].size() == size_t(quiet::kColLanes), "quiet_window: 64 records per tile");
            r[i] = rec[i].empty() ? nullptr : rec[i].data();
          }
          return (unsigned long long)quiet::window(r, words.data(), own_l, own, own_r);
        },
        py::arg("rec"), py::arg("words"), py::arg("own_l"), py::arg("own"), py::arg("own_r"));
  py::class_<quiet::ColsModel>(m, "QuietColsModel")
      .def(py::init<int, int, int, int, int>(), py::arg("ncolw"), py::arg("nseg"), py::arg("T"), py::arg("last_own"),
           py::arg("g"))
      .def("block", [](quiet::ColsModel& c, const std::vector<uint32_t>& fresh, bool follow, bool cols) {
             std::vector<unsigned long long> out;
             for (uint64_t v : c.block(fresh, follow, cols)) out.push_back(v);
             return out;
           },
           py::arg("fresh"), py::arg("follow"), py::arg("cols"))
      .def("window_of", [](const quiet::ColsModel& c, int t) { return (unsigned long long)c.window_of(t); })
      .def("words", [](const quiet::ColsModel& c) { return c.list().words(); })
      .def("candidates", [](const quiet::ColsModel& c) { return c.list().candidates(); })
      .def("records", &quiet::ColsModel::records)
      .def("valid", &quiet::ColsModel::valid);
  py::class_<quiet::Launch>(m, "QuietLaunch")
      .def(py::init([](std::uintptr_t in, std::uintptr_t out, int T, int64_t row_lo, int64_t row_hi, int64_t pitch,
                       int ncolw, int nseg, int seg_rows, int seg_rem, int grp_q, int wrap_w) {
             return quiet::Launch{reinterpret_cast<const void*>(in), reinterpret_cast<const void*>(out), T, row_lo,
                                  row_hi, pitch, ncolw, nseg, seg_rows, seg_rem, grp_q, wrap_w};
           }),
           py::arg("inp"), py::arg("out"), py::arg("T") = 12, py::arg("row_lo") = 32, py::arg("row_hi") = 800,
           py::arg("pitch") = 768, py::arg("ncolw") = 3, py::arg("nseg") = 8, py::arg("seg_rows") = 96,
           py::arg("seg_rem") = 0, py::arg("grp_q") = 27, py::arg("wrap_w") = 160);
  m.def("quiet_may_follow", &quiet::may_follow);
  py::class_<quiet::Policy>(m, "QuietPolicy")
      .def(py::init([](int mode, int scout, int on, int off) {
             quiet::Policy p;
             p.mode = mode;
             p.scout = scout;
             p.on = on;
             p.off = off;
             return p;
           }),
           py::arg("mode") = -1, py::arg("scout") = 128, py::arg("on") = 60, py::arg("off") = 35)
      .def("next", &quiet::Policy::next)
      .def("ran", &quiet::Policy::ran)
      .def("report", &quiet::Policy::report)
      .def("name", &quiet::Policy::name)
      .def_readonly("skipping", &quiet::Policy::skipping)
      .def_readonly("blocks_dense", &quiet::Policy::blocks_dense)
      .def_readonly("blocks_scout", &quiet::Policy::blocks_scout)
      .def_readonly("blocks_skip", &quiet::Policy::blocks_skip);

  // ---- I/O ----
  m.def("read_text_tile", [](const std::string& path, int64_t W, int64_t H, int64_t r0, int64_t r1,
                             int64_t c0, int64_t c1) {
    std::vector<uint8_t> out;
    {
      py::gil_scoped_release rel;
      read_text_tile(path, W, H, {r0, r1}, {c0, c1}, out);
    }
    return to_array(std::move(out), r1 - r0, c1 - c0);
  });
  m.def("read_text_grid", [](const std::string& path, int64_t W, int64_t H) {
    std::vector<uint8_t> out;
    {
      py::gil_scoped_release rel;
      read_text_grid(path, W, H, out);
    }
    return to_array(std::move(out), H, W);
  });
  m.def("create_text_file", &create_text_file, py::call_guard<py::gil_scoped_release>());
  m.def("write_text_tile",
        [](const std::string& path, int64_t W, int64_t H, int64_t r0, int64_t c0,
           py::array_t<uint8_t, py::array::c_style | py::array::forcecast> a) {
          GOL_REQUIRE(a.ndim() == 2, "expected a 2-D array");
          int64_t nr = a.shape(0), nc = a.shape(1);
          const uint8_t* p = a.data();
          py::gil_scoped_release rel;
          write_text_tile(path, W, H, {r0, r0 + nr}, {c0, c0 + nc}, p, nc);
        });
  m.def("write_text_grid", [](const std::string& path, py::array_t<uint8_t, py::array::c_style | py::array::forcecast> a) {
    GOL_REQUIRE(a.ndim() == 2, "expected a 2-D array");
    int64_t H = a.shape(0), W = a.shape(1);
    const uint8_t* p = a.data();
    py::gil_scoped_release rel;
    write_text_grid(path, W, H, p);
  });
  m.def("parse_rle", [](const std::string& text) {
    RlePattern p = parse_rle(text);
    const int64_t h = p.h, w = p.w;
    return py::make_tuple(to_array(std::move(p.cells), h, w), p.rule);
  });
  m.def("format_rle",
        [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> a, const std::string& rule) {
          GOL_REQUIRE(a.ndim() == 2, "expected a 2-D array");
          return format_rle(a.data(), a.shape(1), a.shape(0), rule);
        },
        py::arg("cells"), py::arg("rule") = "B3/S23");
  m.attr("DENSITY_BLOCKS_MAX") = Backend::kDensityBlocksMax;
  m.attr("WINDOW_CELLS_MAX") = Backend::kWindowCellsMax;
  m.def("generate_text_file", &generate_text_file, py::arg("path"), py::arg("W"), py::arg("H"),
        py::arg("seed") = 1, py::arg("density") = 0.5, py::call_guard<py::gil_scoped_release>());
  m.def("random_grid", [](int64_t W, int64_t H, uint64_t seed, double density) {
    std::vector<uint8_t> v(size_t(W * H));
    uint32_t th = density_thresh(density);
    for (int64_t r = 0; r < H; ++r)
      for (int64_t x = 0; x < W; ++x) v[size_t(r * W + x)] = uint8_t(rng_cell(seed, r, x, th));
    return to_array(std::move(v), H, W);
  }, py::arg("W"), py::arg("H"), py::arg("seed") = 1, py::arg("density") = 0.5);

  // ---- batched small universes (gol/batch.hpp) ----
  // grids: a (B, H, W) uint8 array of 0/1, or None with batch / shape / seed /
  // density (universe b is random_grid(W, H, seed + b, density)).  Returns
  // (generations, period, stop, population, grids or None, kernel_ms, variant).
  m.attr("BATCH_STOP") = py::make_tuple(kBatchStopNames[0], kBatchStopNames[1], kBatchStopNames[2]);
  m.def("simulate_batch",
        [](std::optional<py::array_t<uint8_t, py::array::c_style | py::array::forcecast>> grids, int64_t batch,
           int W, int H, uint64_t seed, double density, int64_t max_gens, int64_t max_period,
           const std::string& rule, const std::string& boundary, const std::string& engine, bool return_grids,
           int threads, int device, std::optional<Tuning> tune, const std::vector<std::string>& rules,
           int64_t soups, bool share_soups, bool clusters) -> py::tuple {
          BatchConfig cfg;
          cfg.clusters = clusters;
          BatchInput in;
          for (size_t r = 0; r < rules.size(); ++r) {
            try {
              cfg.rules.push_back(parse_rule(rules[r]));
            } catch (const std::exception& e) {
              throw Error("batch: rule " + std::to_string(r) + " of the list: " + e.what());
            }
          }
          cfg.soups_per_rule = soups;
          cfg.share_soups = share_soups;
          if (grids) {
            GOL_REQUIRE(grids->ndim() == 3, "batch: the grids are a (B, H, W) uint8 array, got " +
                                                std::to_string(grids->ndim()) + " dimensions");
            in.B = grids->shape(0);
            // Shared soups: the K grids serve every rule (validate_batch checks K).
            if (!cfg.rules.empty() && share_soups && in.B == soups) in.B = int64_t(cfg.rules.size()) * soups;
            H = int(grids->shape(1));
            W = int(grids->shape(2));
            in.cells = grids->data();
          } else {
            in.B = batch;
            in.seed = seed;
            in.density = density;
          }
          cfg.W = W;
          cfg.H = H;
          cfg.rule = parse_rule(rule);
          cfg.boundary = parse_boundary(boundary);
          cfg.max_gens = max_gens;
          cfg.max_period = max_period;
          cfg.want_grids = return_grids;
          GOL_REQUIRE(engine == "cpu" || engine == "hip", "batch: engine '" + engine + "': cpu or hip");
          BatchResult r;
          {
            py::gil_scoped_release rel;
            r = engine == "hip" ? run_batch_hip(device, cfg, in, tune ? *tune : Tuning::from_env())
                                : run_batch_cpu(threads, cfg, in);
          }
          const py::ssize_t B = py::ssize_t(in.B);
          py::array_t<int32_t> gens(B), per(B), pop(B);
          py::array_t<uint8_t> stop(B);
          std::copy(r.generations.begin(), r.generations.end(), gens.mutable_data());
          std::copy(r.period.begin(), r.period.end(), per.mutable_data());
          std::copy(r.population.begin(), r.population.end(), pop.mutable_data());
          std::copy(r.stop.begin(), r.stop.end(), stop.mutable_data());
          py::object cells = py::none();
          if (return_grids) {
            auto* heap = new std::vector<uint8_t>(std::move(r.grids));
            py::capsule owner(heap, [](void* p) { delete static_cast<std::vector<uint8_t>*>(p); });
            cells = py::array_t<uint8_t>({int64_t(B), int64_t(H), int64_t(W)},
                                         {int64_t(H) * W, int64_t(W), int64_t(1)}, heap->data(), owner);
          }
          if (clusters)
            return py::make_tuple(gens, per, stop, pop, cells, r.kernel_ms, r.variant, census_arrays(r.census));
          return py::make_tuple(gens, per, stop, pop, cells, r.kernel_ms, r.variant);
        },
        py::arg("grids") = py::none(), py::arg("batch") = 0, py::arg("W") = 64, py::arg("H") = 64,
        py::arg("seed") = 1, py::arg("density") = 0.5, py::arg("max_gens") = 1024, py::arg("max_period") = 64,
        py::arg("rule") = "B3/S23", py::arg("boundary") = "torus", py::arg("engine") = "cpu",
        py::arg("return_grids") = false, py::arg("threads") = 0, py::arg("device") = 0,
        py::arg("tune") = py::none(), py::arg("rules") = std::vector<std::string>{}, py::arg("soups") = 1,
        py::arg("share_soups") = false, py::arg("clusters") = false);

  // The cluster census of arbitrary grids (B, H, W) of a batch shape: (clusters per universe, universe,
  // signature, cells, height, width, spanning, ms, count_ms).
  m.def("find_clusters",
        [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> grids, const std::string& boundary,
           const std::string& engine, int threads, int device, std::optional<Tuning> tune) -> py::tuple {
          GOL_REQUIRE(grids.ndim() == 3, "find_clusters: the grids are a (B, H, W) uint8 array, got " +
                                             std::to_string(grids.ndim()) + " dimensions");
          GOL_REQUIRE(engine == "cpu" || engine == "hip", "find_clusters: engine '" + engine + "': cpu or hip");
          const int64_t B = grids.shape(0);
          const int H = int(std::min<int64_t>(grids.shape(1), 1 << 20)), W = int(std::min<int64_t>(grids.shape(2), 1 << 20));
          const Boundary bd = parse_boundary(boundary);
          const uint8_t* cells = grids.data();
          ClusterCensus c;
          {
            py::gil_scoped_release rel;
            c = engine == "hip" ? find_clusters_hip(device, W, H, bd, B, cells, tune ? *tune : Tuning::from_env())
                                : find_clusters_cpu(threads, W, H, bd, B, cells);
          }
          return census_arrays(c);
        },
        py::arg("grids"), py::arg("boundary") = "torus", py::arg("engine") = "cpu", py::arg("threads") = 0,
        py::arg("device") = 0, py::arg("tune") = py::none());
  m.def("cluster_signature", [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> cells) {
    GOL_REQUIRE(cells.ndim() == 2, "cluster_signature: expected a 2-D array");
    return cluster_signature(cells.data(), cells.shape(1), cells.shape(0));
  });
  m.def("cluster_name", &cluster_name);
  // The exclusive scan every engine applies to the per-universe counts (refuses more than 2^28 records).
  m.def("cluster_offsets", [](const std::vector<int32_t>& counts) {
    std::vector<int32_t> offsets;
    const int64_t total = cluster_offsets(counts, offsets);
    return py::make_tuple(total, offsets);
  });
  m.attr("CLUSTER_RECORDS_MAX") = kClusterRecordsMax;

  // ---- serial reference (src/game.c semantics) ----
  m.def("cpu_reference_run",
        [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> a, int64_t gen_limit,
           bool check_similarity, int sim_freq, int threads, const std::string& rule, const std::string& boundary,
           bool census, bool fingerprint) -> py::tuple {
          GOL_REQUIRE(a.ndim() == 2, "expected a 2-D array");
          int64_t H = a.shape(0), W = a.shape(1);
          std::vector<uint8_t> g(a.data(), a.data() + W * H);
          const Rule rl = parse_rule(rule);
          const Boundary bd = parse_boundary(boundary);
          RefResult r;
          {
            py::gil_scoped_release rel;
            r = cpu_reference_run(g, W, H, gen_limit, check_similarity, sim_freq, threads, rl, bd, census,
                                  fingerprint);
          }
          // (generations, ms, grid), then the population if asked for, then the fingerprints if asked for.
          py::list out;
          out.append(r.generations);
          out.append(r.loop_ms);
          out.append(to_array(std::move(g), H, W));
          if (census) {
            py::array_t<int64_t> pop(static_cast<py::ssize_t>(r.population.size()));
            std::copy(r.population.begin(), r.population.end(), pop.mutable_data());
            out.append(pop);
          }
          if (fingerprint) {
            py::array_t<uint64_t> fp(static_cast<py::ssize_t>(r.fingerprint.size()));
            std::copy(r.fingerprint.begin(), r.fingerprint.end(), fp.mutable_data());
            out.append(fp);
          }
          return py::tuple(out);
        },
        py::arg("grid"), py::arg("gen_limit") = 1000, py::arg("check_similarity") = true,
        py::arg("sim_freq") = 3, py::arg("threads") = 1, py::arg("rule") = "B3/S23",
        py::arg("boundary") = "torus", py::arg("census") = false, py::arg("fingerprint") = false);
  // The grid fingerprint of an H x W array of cells (gol/fingerprint.hpp), on the host.
  m.def("grid_fingerprint", [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> a) {
    GOL_REQUIRE(a.ndim() == 2, "expected a 2-D array");
    return grid_fingerprint(a.data(), a.shape(1), a.shape(1), a.shape(0));
  });

  // ---- bitop3 / rule emulation (for kernel-level tests) ----
  m.def("rule_words", [](uint32_t a0, uint32_t a1, uint32_t a2, uint32_t b0, uint32_t b1, uint32_t b2,
                         uint32_t c0, uint32_t c1, uint32_t c2) {
    return rule_host(hsum_host(a0, a1, a2), hsum_host(b0, b1, b2), hsum_host(c0, c1, c2), b1);
  });
  // The same through the general form (rule_host(Rule, ...)), any rule.
  m.def("rule_words_for", [](const std::string& rule, uint32_t a0, uint32_t a1, uint32_t a2, uint32_t b0, uint32_t b1,
                             uint32_t b2, uint32_t c0, uint32_t c1, uint32_t c2) {
    return rule_host(parse_rule(rule), hsum_host(a0, a1, a2), hsum_host(b0, b1, b2), hsum_host(c0, c1, c2), b1);
  });
  // Exhaustive check of the table derivation (rule_tables): the general host
  // form on all 512 3x3 neighbourhoods (packed one per bit into 16 words) for
  // every rule without B0, against the plain definition.  Returns
  // (rules checked, disagreeing (rule, neighbourhood) pairs).
  m.def("rule_tables_check", []() {
    py::gil_scoped_release rel;
    uint32_t plane[9][16] = {};
    for (int i = 0; i < 512; ++i)
      for (int k = 0; k < 9; ++k)
        if ((i >> k) & 1) plane[k][i / 32] |= 1u << (i % 32);
    HSum hs[3][16];
    for (int r = 0; r < 3; ++r)
      for (int w = 0; w < 16; ++w)
        hs[r][w] = {bop3_host<tt::XOR3>(plane[3 * r][w], plane[3 * r + 1][w], plane[3 * r + 2][w]),
                    bop3_host<tt::MAJ>(plane[3 * r][w], plane[3 * r + 1][w], plane[3 * r + 2][w])};
    int64_t rules = 0, bad = 0;
    for (unsigned b = 0; b < 512; b += 2)  // no B0
      for (unsigned s = 0; s < 512; ++s) {
        const Rule rule{uint16_t(b), uint16_t(s)};
        ++rules;
        for (int w = 0; w < 16; ++w) {
          const uint32_t got = rule_host(rule, hs[0][w], hs[1][w], hs[2][w], plane[4][w]);
          uint32_t want = 0;
          for (int j = 0; j < 32; ++j) {
            const int i = 32 * w + j, ctr = (i >> 4) & 1, n = __builtin_popcount(unsigned(i)) - ctr;
            want |= uint32_t(((ctr ? s : b) >> n) & 1u) << j;
          }
          bad += __builtin_popcount(got ^ want);
        }
      }
    return std::make_pair(rules, bad);
  });
}
