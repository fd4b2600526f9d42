// pybind11 binding of csrc/iocopy_core.h: the bulk copy engine (io_uring
// small-file batching + copy_file_range), exposed to Python as
// gpu_docker_api_amd.ops._iocopy. Everything but the binding lives in the
// header, which csrc/iocopy_selftest.cpp drives stand-alone.
#include <pybind11/pybind11.h>

#include "iocopy_core.h"

namespace py = pybind11;

namespace {

py::dict copy_tree(const std::string& src, const std::string& dst, bool use_uring,
                   bool use_copy_file_range) {
  iocopy::Options opt;
  opt.use_uring = use_uring;
  opt.use_copy_file_range = use_copy_file_range;
  iocopy::CopyStats stats;
  {
    py::gil_scoped_release rel;  // the walk does blocking IO
    stats = iocopy::copy_tree(src, dst, opt);
  }
  py::dict out;
  out["files"] = stats.files;
  out["dirs"] = stats.dirs;
  out["symlinks"] = stats.symlinks;
  out["specials"] = stats.specials;
  out["bytes"] = stats.bytes;
  out["io_uring"] = stats.used_uring;
  return out;
}

}  // namespace

PYBIND11_MODULE(_iocopy, m) {
  m.doc() = "bulk copy engine: io_uring small-file batching + copy_file_range";
  m.def("copy_tree", &copy_tree, py::arg("src"), py::arg("dst"), py::kw_only(),
        py::arg("use_uring") = true, py::arg("use_copy_file_range") = true);
  m.def("uring_available", &iocopy::uring_available);
}
