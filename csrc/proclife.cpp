// pybind11 binding of csrc/proclife_core.h: the proc runtime's spawn, reap,
// teardown and small-file writes as gpu_docker_api_amd.ops._proclife.
//
// Strings cross as os.fsencode would encode them (PyUnicode_FSConverter), so
// an argv or env entry with a surrogate-escaped byte spawns exactly what
// subprocess would have spawned. OSError carries the errno, so ENOENT is a
// FileNotFoundError and EACCES a PermissionError on the Python side.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstdio>
#include <memory>

#include "proclife_core.h"

namespace py = pybind11;
namespace pl = proclife;

namespace {

pl::BaseEnv g_base_env;

std::string fsbytes(py::handle h, const char* what) {
  PyObject* raw = nullptr;
  if (!PyUnicode_FSConverter(h.ptr(), &raw)) throw py::error_already_set();
  py::bytes b = py::reinterpret_steal<py::bytes>(raw);
  std::string s = b;
  if (s.find('\0') != std::string::npos)
    throw py::value_error(std::string("embedded null byte in ") + what);
  return s;
}

std::vector<pl::KV> env_items(py::handle mapping) {
  std::vector<pl::KV> out;
  if (mapping.is_none()) return out;
  py::object items = py::isinstance<py::dict>(mapping)
                         ? py::reinterpret_borrow<py::dict>(mapping).attr("items")()
                         : py::reinterpret_borrow<py::object>(mapping);
  for (py::handle it : items) {
    py::tuple kv = py::reinterpret_borrow<py::tuple>(it);
    std::string k = fsbytes(kv[0], "environment");
    if (k.find('=') != std::string::npos)
      throw py::value_error("illegal environment variable name");
    out.emplace_back(std::move(k), fsbytes(kv[1], "environment"));
  }
  return out;
}

[[noreturn]] void raise_oserror(int err, const std::string& filename) {
  errno = err;
  if (filename.empty())
    PyErr_SetFromErrno(PyExc_OSError);
  else
    PyErr_SetFromErrnoWithFilename(PyExc_OSError, filename.c_str());
  throw py::error_already_set();
}

class PyChild {
 public:
  explicit PyChild(pl::Child&& c) : c_(std::move(c)), pid_(c_.pid) {}

  int pid() const { return pid_; }
  unsigned long long starttime() const { return c_.starttime; }
  py::object returncode() const {
    return c_.exited ? py::cast(c_.returncode) : py::none();
  }
  py::object poll() {
    return c_.poll() ? py::cast(c_.returncode) : py::none();
  }
  py::object wait(py::object timeout) {
    int ms = timeout.is_none() ? -1 : static_cast<int>(timeout.cast<double>() * 1000.0);
    bool done;
    {
      py::gil_scoped_release nogil;
      done = c_.wait(ms);
    }
    return done ? py::cast(c_.returncode) : py::none();
  }
  int fileno() const { return c_.pidfd; }
  void close() { c_.close_fd(); }

 private:
  pl::Child c_;
  int pid_;
};

std::unique_ptr<PyChild> spawn(py::sequence argv, py::object cwd, py::object env_overrides,
                               py::object log_path) {
  std::vector<std::string> args;
  for (py::handle a : argv) args.push_back(fsbytes(a, "argv"));
  if (args.empty()) throw py::value_error("empty argv");
  std::string cwd_s = fsbytes(cwd, "cwd"), log_s = fsbytes(log_path, "log_path");
  std::vector<pl::KV> over = env_items(env_overrides);
  pl::Child child;
  pl::SpawnError res;
  {
    py::gil_scoped_release nogil;
    res = pl::spawn(args, cwd_s, g_base_env, over, log_s, &child);
  }
  if (res.err) raise_oserror(res.err, res.filename);
  return std::make_unique<PyChild>(std::move(child));
}

}  // namespace

PYBIND11_MODULE(_proclife, m) {
  m.doc() = "container process lifecycle on raw syscalls (csrc/proclife_core.h)";

  py::class_<PyChild>(m, "Child")
      .def_property_readonly("pid", &PyChild::pid)
      .def_property_readonly("starttime", &PyChild::starttime)
      .def_property_readonly("returncode", &PyChild::returncode)
      .def("poll", &PyChild::poll)
      .def("wait", &PyChild::wait, py::arg("timeout") = py::none())
      .def("fileno", &PyChild::fileno)
      .def("close", &PyChild::close);

  m.def(
      "set_base_env",
      [](py::object mapping) {
        g_base_env.set(env_items(mapping));
        return g_base_env.size();
      },
      py::arg("env"), "snapshot and encode the base environment once");
  m.def("base_env_size", [] { return g_base_env.size(); });
  m.def("spawn", &spawn, py::arg("argv"), py::arg("cwd"), py::arg("env_overrides"),
        py::arg("log_path"));
  m.def("proc_starttime", [](int pid) { return pl::read_starttime(pid); }, py::arg("pid"));
  m.def(
      "remove_tree",
      [](py::object path) {
        std::string p = fsbytes(path, "path");
        long failed;
        {
          py::gil_scoped_release nogil;
          failed = pl::remove_tree(p.c_str());
        }
        return failed;
      },
      py::arg("path"));
  m.def(
      "prepare_container_dir",
      [](py::object cdir, py::object spec_json) {
        std::string d = fsbytes(cdir, "cdir"), failed;
        std::string data = spec_json.cast<std::string>();  // str (UTF-8) or bytes
        if (int e = pl::prepare_container_dir(d, data.data(), data.size(), &failed))
          raise_oserror(e, failed);
      },
      py::arg("cdir"), py::arg("spec_json"));
  m.def(
      "write_file",
      [](py::object path, py::object data) {
        std::string p = fsbytes(path, "path");
        std::string d = data.cast<std::string>();  // str (UTF-8) or bytes
        if (int e = pl::write_file(p.c_str(), d.data(), d.size())) raise_oserror(e, p);
      },
      py::arg("path"), py::arg("data"));
}
