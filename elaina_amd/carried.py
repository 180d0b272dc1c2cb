"""The selections, the per-pixel state and the adaptive solves of the carried frame solve (wost_solve_more_where & co.,
include/wost.h), shared by UniformIntegrator and UniformIntegrator3: the two differ in the prefix of the entry points."""
import ctypes as C

import numpy as np

from .capi import Adaptive, Stats, _check, _fp, _ip


class CarriedSolves:
    """mixed into an integrator with .lib, ._handle, .n_pixels and ._prefix ("wost_" or "wost3_")"""

    def _carried_fn(self, name):
        return getattr(self.lib, self._prefix + name), self._prefix + name

    def solve_more_where(self, more_spp, select=None):
        """more_spp samples on the pixels whose entry in select (n_pixels values, nonzero = continue) is set; None: every
        pixel, which is solve_more.  Every pixel's field at its own count is in self.solution; returns wall milliseconds"""
        fn, name = self._carried_fn("solve_more_where")
        field = np.zeros((self.n_pixels, 3), dtype=np.float32)
        st = Stats()
        sel = None
        if select is not None:
            sel = np.ascontiguousarray(np.asarray(select).reshape(-1) != 0, dtype=np.uint8)
            if sel.size != self.n_pixels:
                raise ValueError("select has %d entries, the frame %d pixels" % (sel.size, self.n_pixels))
        ptr = sel.ctypes.data_as(C.POINTER(C.c_uint8)) if sel is not None else None
        _check(fn(self._handle, int(more_spp), ptr, _fp(field), C.byref(st)), name)
        self.solution = field
        self.last_stats = st.as_dict()
        return int(st.solve_ms)

    def solve_more_where_sharded(self, shard_index, shard_count, more_spp, select_dev_ptr, field_dev_ptr, stream_ptr=None):
        """the same for one shard on device pointers (ints): n_pixels bytes of selection (0: every pixel), a zero-filled field"""
        fn, name = self._carried_fn("solve_more_where_sharded")
        st = Stats()
        _check(fn(self._handle, shard_index, shard_count, int(more_spp), C.c_void_p(select_dev_ptr or 0), C.c_void_p(field_dev_ptr),
                  C.c_void_p(stream_ptr or 0), C.byref(st)), name)
        self.last_stats = st.as_dict()
        return self.last_stats

    def carried(self):
        """the per-pixel state of the carried solve: {"spp": samples done, "batches": calls that walked the pixel, "sum": the
        raw sums (n, 3), "stderr": the batch-means standard error of sum / spp (n, 3), +inf below two batches}"""
        fn, name = self._carried_fn("solve_carried")
        out = {"spp": np.zeros(self.n_pixels, np.int32), "batches": np.zeros(self.n_pixels, np.int32),
               "sum": np.zeros((self.n_pixels, 3), np.float32), "stderr": np.zeros((self.n_pixels, 3), np.float32)}
        _check(fn(self._handle, _ip(out["spp"]), _ip(out["batches"]), _fp(out["sum"]), _fp(out["stderr"])), name)
        return out

    def _adaptive(self, batch_spp, max_spp, abs_tol, rel_tol, min_batches):
        return Adaptive(int(batch_spp), int(min_batches), int(max_spp), float(abs_tol), float(rel_tol))

    def solve_adaptive(self, batch_spp, max_spp, abs_tol=0.0, rel_tol=0.0, min_batches=4):
        """batches of batch_spp samples on the pixels whose standard error is above max(abs_tol, rel_tol * |mean|) in some
        channel (or that have fewer than min_batches batches) and that have room under max_spp, until none is left; starts from
        the carried solve as it stands.  The field is in self.solution, the standard errors in self.stderr, the per-pixel
        sample counts in self.spp_map; returns wall milliseconds"""
        fn, name = self._carried_fn("solve_adaptive")
        field = np.zeros((self.n_pixels, 3), dtype=np.float32)
        se = np.zeros((self.n_pixels, 3), dtype=np.float32)
        spp = np.zeros(self.n_pixels, dtype=np.int32)
        st = Stats()
        a = self._adaptive(batch_spp, max_spp, abs_tol, rel_tol, min_batches)
        _check(fn(self._handle, C.byref(a), _fp(field), _fp(se), _ip(spp), C.byref(st)), name)
        self.solution, self.stderr, self.spp_map = field, se, spp
        self.last_stats = st.as_dict()
        return int(st.solve_ms)

    def solve_adaptive_sharded(self, shard_index, shard_count, batch_spp, max_spp, field_dev_ptr, stream_ptr=None, abs_tol=0.0, rel_tol=0.0,
                               min_batches=4):
        """the same for one shard into a zero-filled device field"""
        fn, name = self._carried_fn("solve_adaptive_sharded")
        st = Stats()
        a = self._adaptive(batch_spp, max_spp, abs_tol, rel_tol, min_batches)
        _check(fn(self._handle, shard_index, shard_count, C.byref(a), C.c_void_p(field_dev_ptr), C.c_void_p(stream_ptr or 0), C.byref(st)), name)
        self.last_stats = st.as_dict()
        return self.last_stats
