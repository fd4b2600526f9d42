"""Native ops: HIP/CDNA4 kernels, the io_uring copy engine and the proc
runtime's lifecycle module (spawn / reap / teardown).

Built in-tree by :mod:`.build` (the .so files live next to this file so they
travel to GPU boxes with the repo snapshot). On a GPU box these MUST load —
ops fail loudly rather than falling back to a silent eager path.
"""
