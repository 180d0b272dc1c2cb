"""What UniformIntegrator and UniformIntegrator3 have in common: every method whose entry points exist as wost_* and wost3_*
(include/wost.h) with the same arguments -- the frame solve, the point solves, the carried solve with its selections and
adaptive variant, the batch queries.  The two classes differ in the prefix of the entry points and in the columns of a point."""
import ctypes as C

import numpy as np

from . import capi
from .capi import Adaptive, Stats, _check, _fp, _ip


class UniformCalls:
    """base of an integrator with .lib, ._handle, .n_pixels, .settings, ._prefix ("wost_" or "wost3_") and ._dim (2 or 3)"""

    def _fn(self, name):
        return getattr(self.lib, self._prefix + name), self._prefix + name

    def _host_solve(self, entry, n, *args):
        """a host entry point whose last arguments are an (n, 3) field and the stats -> (field, stats)"""
        fn, name = self._fn(entry)
        field = np.zeros((n, 3), dtype=np.float32)
        st = Stats()
        _check(fn(self._handle, *args, _fp(field), C.byref(st)), name)
        self.last_stats = st.as_dict()
        return field, st

    def _dev_solve(self, entry, *args):
        """an entry point on device pointers whose last argument is the stats -> the stats as a dict"""
        fn, name = self._fn(entry)
        st = Stats()
        _check(fn(self._handle, *args, C.byref(st)), name)
        self.last_stats = st.as_dict()
        return self.last_stats

    def _points(self, a):
        """an array of points as the entry points read it; the 2-D queries take the caller's array as it is"""
        p = np.ascontiguousarray(a, dtype=np.float32)
        return p if self._dim == 2 else p.reshape(-1, 3)

    def _seed_width(self, seed_width):
        return int(self.settings.frameSize[0] if seed_width is None else seed_width)

    # -- reference surface ------------------------------------------------------------------
    def solve(self, pixel_begin=0, pixel_end=None):
        """returns wall milliseconds like the reference; the field is in self.solution"""
        if pixel_end is None:
            pixel_end = self.n_pixels
        self.solution, st = self._host_solve("solve", pixel_end - pixel_begin, pixel_begin, pixel_end)
        return int(st.solve_ms)

    def solve_sharded(self, shard_index, shard_count, field_dev_ptr, stream_ptr=None):
        """field_dev_ptr: device pointer (int) to a zero-filled width*height*3 float buffer"""
        return self._dev_solve("solve_sharded", shard_index, shard_count, C.c_void_p(field_dev_ptr), C.c_void_p(stream_ptr or 0))

    def solve_points(self, points, seed_base=0, seed_width=None):
        """the solve at the caller's evaluation points ([n, dim] floats) instead of the frame's pixels (wost_solve_points,
        wost3_solve_points): point i runs on the random stream of pixel seed_base + i in a frame seed_width wide (default: the
        frame's width); returns the (n, 3) float32 field"""
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, self._dim)
        return self._host_solve("solve_points", len(p), _fp(p), len(p), int(seed_base), self._seed_width(seed_width))[0]

    def solve_points_dev(self, points_ptr, n, field_ptr, stream_ptr=None, seed_base=0, seed_width=None):
        """the same on device pointers (ints): n * dim floats of points, n * 3 floats of field, on the caller's stream"""
        return self._dev_solve("solve_points_dev", C.c_void_p(points_ptr), int(n), int(seed_base), self._seed_width(seed_width),
                               C.c_void_p(field_ptr), C.c_void_p(stream_ptr or 0))

    # -- the gradient at the caller's points (wost_solve_gradient_points & co.) -------------------
    GRADIENT_OUTPUTS = ("stderr", "field", "radius", "first_pts")

    def _gradient_seeds(self, n, seed_base, walk_seed_base, seed_width):
        seed_base = int(seed_base)
        return seed_base, int(seed_base + n if walk_seed_base is None else walk_seed_base), self._seed_width(seed_width)

    def solve_gradient_points(self, points, seed_base=0, walk_seed_base=None, seed_width=None, want=("stderr", "field", "radius"), spp=None):
        """grad u at the caller's points ([n, dim] floats) by the walk-on-spheres estimator with spp walks per point
        (wost_solve_gradient_points, wost3_solve_gradient_points; include/wost.h has the estimator).  Point i draws its directions
        from the stream of pixel seed_base + i, its walks run on the streams of pixels walk_seed_base + i * spp + s (default:
        seed_base + n, right behind the directions') in a frame seed_width wide (default: the frame's width).  Returns a dict of
        float32 arrays: "grad" (n, dim, 3) = d u_c / d x_k, and what `want` names of "stderr" (n, dim, 3), "field" (n, 3) the
        mean of the point's walks, "radius" (n,) and "first_pts" (n, spp, dim) -- the last sized by `spp` (default: the spp the
        integrator was made with; pass it after set_option("spp", ...)).  A scene with a source term is refused unless
        set_option("grad_source", 1) was called on the integrator: then grad and stderr include the in-ball term of the
        gradient, from spp more samples per point, and "field" the in-ball term of u"""
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, self._dim)
        n, S = len(p), int(self.settings.samplesPerPixel if spp is None else spp)
        unknown = set(want) - set(self.GRADIENT_OUTPUTS)
        if unknown:
            raise ValueError("unknown gradient outputs %s (known: %s)" % (sorted(unknown), ", ".join(self.GRADIENT_OUTPUTS)))
        shapes = {"grad": (n, self._dim, 3), "stderr": (n, self._dim, 3), "field": (n, 3), "radius": (n,), "first_pts": (n, S, self._dim)}
        out = {k: np.zeros(shapes[k], np.float32) for k in ("grad",) + tuple(k for k in self.GRADIENT_OUTPUTS if k in want)}
        ptr = {k: out[k].ctypes.data if k in out else None for k in shapes}
        go = capi.GradientOut(ptr["grad"], ptr["stderr"], ptr["field"], ptr["radius"], ptr["first_pts"])
        fn, name = self._fn("solve_gradient_points")
        st = Stats()
        _check(fn(self._handle, _fp(p), n, *self._gradient_seeds(n, seed_base, walk_seed_base, seed_width), C.byref(go), C.byref(st)), name)
        self.last_stats = st.as_dict()
        return out

    def solve_gradient_points_dev(self, points_ptr, n, grad_ptr, stream_ptr=None, seed_base=0, walk_seed_base=None, seed_width=None,
                                  stderr_ptr=None, field_ptr=None, radius_ptr=None, first_pts_ptr=None):
        """the same on device pointers (ints) on the caller's stream: n * dim floats of points, n * dim * 3 of grad and, where
        given, n * dim * 3 of stderr, n * 3 of field, n of radius, n * spp * dim of first points; a point with a non-finite
        coordinate is never walked and answers NaN in every output.  Returns the stats as a dict"""
        go = capi.GradientOut(grad_ptr, stderr_ptr or None, field_ptr or None, radius_ptr or None, first_pts_ptr or None)
        return self._dev_solve("solve_gradient_points_dev", C.c_void_p(points_ptr), int(n),
                               *self._gradient_seeds(int(n), seed_base, walk_seed_base, seed_width), C.byref(go), C.c_void_p(stream_ptr or 0))

    # -- the carried gradient list (wost_gradient_points_carry & co.) ---------------------------
    def _gradient_carry_args(self, n, batch_walks, round_stride, max_rounds, seed_base, walk_seed_base, seed_width):
        n, seed_base, max_rounds = int(n), int(seed_base), int(max_rounds)
        stride = n if round_stride is None else int(round_stride)
        # the walks' seeds by default: just behind the direction seeds of the last round
        walk = seed_base + (max_rounds - 1) * stride + n if walk_seed_base is None else int(walk_seed_base)
        return n, int(batch_walks), stride, max_rounds, seed_base, walk, self._seed_width(seed_width)

    def gradient_points_carry(self, points, batch_walks, round_stride=None, max_rounds=64, seed_base=0, walk_seed_base=None, seed_width=None):
        """bind a list of points ([n, dim] floats) whose gradient is estimated in batches of batch_walks walks per point
        (wost_gradient_points_carry; include/wost.h has the rules): in round r point i draws its directions from the stream of
        pixel seed_base + r * round_stride + i and walks on the streams of pixels walk_seed_base + (r * round_stride + i) *
        batch_walks + s.  round_stride defaults to n, walk_seed_base to just behind the direction seeds of the last of the
        max_rounds rounds.  A rank that holds points [a, b) of a longer list binds them with seed_base + a, walk_seed_base + a *
        batch_walks and the round_stride of the whole list.  The list replaces the one bound before; an empty list releases it.
        On a scene with a source term the bind needs set_option("grad_source", 1), as solve_gradient_points does; the list keeps
        the option's value of the bind for all its rounds."""
        fn, name = self._fn("gradient_points_carry")
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, self._dim)
        _check(fn(self._handle, _fp(p), *self._gradient_carry_args(len(p), batch_walks, round_stride, max_rounds, seed_base, walk_seed_base, seed_width)),
               name)

    def gradient_points_carry_dev(self, points_ptr, n, batch_walks, stream_ptr=None, round_stride=None, max_rounds=64, seed_base=0,
                                  walk_seed_base=None, seed_width=None):
        """the same from a device pointer (int) to n * dim floats, copied on the caller's stream; a point with a non-finite
        coordinate is never walked and answers NaN"""
        fn, name = self._fn("gradient_points_carry_dev")
        _check(fn(self._handle, C.c_void_p(points_ptr), *self._gradient_carry_args(n, batch_walks, round_stride, max_rounds, seed_base, walk_seed_base,
                                                                                  seed_width), C.c_void_p(stream_ptr or 0)), name)

    def _gradient_progress(self):
        fn, name = self._fn("gradient_points_progress")
        n, rounds = C.c_int32(0), C.c_int32(0)
        _check(fn(self._handle, C.byref(n), C.byref(rounds)), name)
        return n.value, rounds.value

    @property
    def gradient_points_done(self):
        """(points of the bound gradient list, rounds done since it was bound or restarted); (0, 0): none is bound"""
        return self._gradient_progress()

    def _gradient_carried_host(self, entry, *args, stats=True):
        """a host entry point of the list whose last arguments are the outputs and, with `stats`, the stats -> the state as a
        dict of arrays: "grad" and "stderr" (n, dim, 3), "field" (n, 3), "radius" (n,), float32, and "batches" (n,) int32"""
        fn, name = self._fn(entry)
        n = self._gradient_progress()[0]
        m = max(n, 1)      # (with no list bound the call says so; its pointers are still real ones)
        out = {"grad": np.zeros((m, self._dim, 3), np.float32), "stderr": np.zeros((m, self._dim, 3), np.float32),
               "field": np.zeros((m, 3), np.float32), "radius": np.zeros(m, np.float32), "batches": np.zeros(m, np.int32)}
        go = capi.GradientCarriedOut(*[out[k].ctypes.data for k in ("grad", "stderr", "field", "radius", "batches")])
        st = Stats()
        _check(fn(self._handle, *args, C.byref(go), *([C.byref(st)] if stats else [])), name)
        if stats:
            self.last_stats = st.as_dict()
        return {k: v[:n] for k, v in out.items()}

    def _select_ptr(self, select, n):
        if select is None:
            return None, None
        sel = np.ascontiguousarray(np.asarray(select).reshape(-1) != 0, dtype=np.uint8)
        if sel.size != n:
            raise ValueError("select has %d entries, the list %d points" % (sel.size, n))
        return sel, sel.ctypes.data_as(C.POINTER(C.c_uint8))

    def gradient_points_more(self, select=None):
        """one batch on the listed points whose entry in select (n values, nonzero = continue) is set and that are walkable;
        None: every walkable point.  Returns the state after the call (the dict of gradient_points_carried)"""
        sel, ptr = self._select_ptr(select, self._gradient_progress()[0])
        return self._gradient_carried_host("gradient_points_more", ptr)

    def gradient_points_carried(self):
        """the state of the list: {"grad", "stderr", "field", "radius", "batches"}; a point no batch has walked answers NaN
        (stderr: +inf below two batches; NaN for a point that is never walked)"""
        return self._gradient_carried_host("gradient_points_carried", stats=False)

    def gradient_points_adaptive(self, max_batches, abs_tol=0.0, rel_tol=0.0, min_batches=4):
        """batches on the walkable points whose standard error is above max(abs_tol, rel_tol * |grad|) in some entry (or that
        have fewer than min_batches batches) and that have room under max_batches, until none is left or the list's rounds
        run out; starts from the state as it stands.  Returns the state after the call"""
        a = capi.GradientAdaptive(int(min_batches), int(max_batches), float(abs_tol), float(rel_tol))
        return self._gradient_carried_host("gradient_points_adaptive", C.byref(a))

    def _gradient_carried_dev(self, grad_ptr, stderr_ptr, field_ptr, radius_ptr, batches_ptr):
        return capi.GradientCarriedOut(grad_ptr, stderr_ptr or None, field_ptr or None, radius_ptr or None, batches_ptr or None)

    def gradient_points_more_dev(self, grad_ptr, select_dev_ptr=None, stream_ptr=None, stderr_ptr=None, field_ptr=None, radius_ptr=None,
                                 batches_ptr=None):
        """gradient_points_more on device pointers (ints) on the caller's stream: n bytes of selection (None: every walkable
        point), n * dim * 3 floats of grad and, where given, of stderr, n * 3 of field, n of radius, n int32 of batches.  Returns
        the stats as a dict"""
        go = self._gradient_carried_dev(grad_ptr, stderr_ptr, field_ptr, radius_ptr, batches_ptr)
        return self._dev_solve("gradient_points_more_dev", C.c_void_p(select_dev_ptr or 0), C.byref(go), C.c_void_p(stream_ptr or 0))

    def gradient_points_adaptive_dev(self, max_batches, grad_ptr, stream_ptr=None, abs_tol=0.0, rel_tol=0.0, min_batches=4, stderr_ptr=None,
                                     field_ptr=None, radius_ptr=None, batches_ptr=None):
        """gradient_points_adaptive into device arrays on the caller's stream"""
        a = capi.GradientAdaptive(int(min_batches), int(max_batches), float(abs_tol), float(rel_tol))
        go = self._gradient_carried_dev(grad_ptr, stderr_ptr, field_ptr, radius_ptr, batches_ptr)
        return self._dev_solve("gradient_points_adaptive_dev", C.byref(a), C.byref(go), C.c_void_p(stream_ptr or 0))

    def gradient_points_restart(self):
        """keep the gradient list, forget its batches and rounds"""
        fn, name = self._fn("gradient_points_restart")
        _check(fn(self._handle), name)

    # -- the exit list (wost_exits_walk & co.) ----------------------------------------------------
    def exits_walk(self, points, walks, walk_seed_base=0, seed_width=None):
        """walk `walks` walks at each of the points ([n, dim] floats) once and keep one exit record per walk on the integrator
        (wost_exits_walk; include/wost.h "Exit lists"): walk (i, s) is solve_points of one sample at point i on the stream of
        pixel walk_seed_base + i * walks + s in a frame seed_width wide (default: the frame's width).  The list replaces the one
        bound before; an empty list releases it.  exits_apply then gives the solution for any Dirichlet colours, exits_adjoint
        its derivative with respect to them.  Returns the stats as a dict"""
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, self._dim)
        return self._dev_solve("exits_walk", _fp(p), len(p), int(walks), int(walk_seed_base), self._seed_width(seed_width))

    def exits_walk_dev(self, points_ptr, n, walks, stream_ptr=None, walk_seed_base=0, seed_width=None):
        """the same from a device pointer (int) to n * dim floats on the caller's stream; a point with a non-finite coordinate
        is never walked and its field is NaN.  Returns the stats as a dict"""
        return self._dev_solve("exits_walk_dev", C.c_void_p(points_ptr), int(n), int(walks), int(walk_seed_base), self._seed_width(seed_width),
                               C.c_void_p(stream_ptr or 0))

    @property
    def exits_done(self):
        """(points of the bound exit list, walks per point); (0, 0): none is bound"""
        fn, name = self._fn("exits_progress")
        n, S = C.c_int32(0), C.c_int32(0)
        _check(fn(self._handle, C.byref(n), C.byref(S)), name)
        return n.value, S.value

    def exits_records(self):
        """the records of the list: {"prim" (n, S) int32: the absorbing segment / triangle by its index in the caller's array,
        -1 for a walk that was not absorbed; "uv" (n, S, dim - 1); "side" (n, S) int32; "thp" (n, S); "base" (n, S, 3)}"""
        fn, name = self._fn("exits_records")
        n, S = self.exits_done
        m = max(n * S, 1)      # (with no list bound the call says so; its pointers are still real ones)
        out = {"prim": np.zeros(m, np.int32), "uv": np.zeros(m * (self._dim - 1), np.float32), "side": np.zeros(m, np.int32),
               "thp": np.zeros(m, np.float32), "base": np.zeros(m * 3, np.float32)}
        rec = capi.ExitRecords(*[out[k].ctypes.data for k in ("prim", "uv", "side", "thp", "base")])
        _check(fn(self._handle, C.byref(rec)), name)
        shapes = {"prim": (n, S), "uv": (n, S, self._dim - 1), "side": (n, S), "thp": (n, S), "base": (n, S, 3)}
        return {k: v[:int(np.prod(shapes[k]))].reshape(shapes[k]) for k, v in out.items()}

    def _exit_verts(self):
        """the vertices of the Dirichlet mesh, which size a set of colours (0: the scene has no such mesh)"""
        prims = getattr(self.problem, "d_segs" if self._dim == 2 else "d_tris", None)
        return 0 if self.problem.d_verts is None or prims is None or len(prims) == 0 else len(self.problem.d_verts)

    def _exit_sets(self, a, rows, cols):
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3 or a.shape[1:] != (rows, cols) or len(a) < 1:
            raise ValueError("expected [K, %d, %d] floats, got %s" % (rows, cols, a.shape))
        return a

    def exits_apply(self, colors, want_stderr=False):
        """the field of the listed points for K sets of Dirichlet colours ([K, n_verts, 6] floats, each in the layout of the
        problem's d_colors; [n_verts, 6] is one set) -> (K, n, 3) float32, or with want_stderr (field, stderr), both (K, n, 3)"""
        fn, name = self._fn("exits_apply")
        c = self._exit_sets(colors, self._exit_verts(), 6)
        K, n = len(c), self.exits_done[0]
        field = np.zeros((K, n, 3), np.float32)
        se = np.zeros((K, n, 3), np.float32) if want_stderr else None
        _check(fn(self._handle, _fp(c), K, _fp(field), _fp(se) if want_stderr else None), name)
        return (field, se) if want_stderr else field

    def exits_apply_dev(self, colors_ptr, K, field_ptr, stream_ptr=None, stderr_ptr=None):
        """the same on device pointers (ints) on the caller's stream: K * n_verts * 6 floats of colours, K * n * 3 of field and,
        where given, of stderr"""
        fn, name = self._fn("exits_apply_dev")
        _check(fn(self._handle, C.c_void_p(colors_ptr), int(K), C.c_void_p(field_ptr), C.c_void_p(stderr_ptr or 0), C.c_void_p(stream_ptr or 0)), name)

    def exits_adjoint(self, dfield):
        """the transposed map of exits_apply: dfield ([K, n, 3] floats; [n, 3] is one set) -> the derivative of sum(field *
        dfield) by the colours, (K, n_verts, 6) float32"""
        fn, name = self._fn("exits_adjoint")
        d = self._exit_sets(dfield, self.exits_done[0], 3)
        out = np.zeros((len(d), self._exit_verts(), 6), np.float32)
        _check(fn(self._handle, _fp(d), len(d), _fp(out)), name)
        return out

    def exits_adjoint_dev(self, dfield_ptr, K, dcolors_ptr, stream_ptr=None):
        """the same on device pointers (ints) on the caller's stream: K * n * 3 floats in, K * n_verts * 6 floats out"""
        fn, name = self._fn("exits_adjoint_dev")
        _check(fn(self._handle, C.c_void_p(dfield_ptr), int(K), C.c_void_p(dcolors_ptr), C.c_void_p(stream_ptr or 0)), name)

    # -- the exit list of the gradient (wost_exits_walk_gradient & co.) ---------------------------
    def exits_walk_gradient(self, points, walks, seed_base=0, walk_seed_base=None, seed_width=None):
        """bind the exit list of the gradient's first points (wost_exits_walk_gradient; include/wost.h "Exit lists of the
        gradient"): radius, directions and first points of the points ([n, dim] floats) as solve_gradient_points(points,
        seed_base, walk_seed_base, seed_width, spp=walks) has them, and one exit record per walk from a first point, walk (i, s)
        on the stream of pixel walk_seed_base + i * walks + s (default: seed_base + n, right behind the directions').  The list
        replaces the one bound before, plain or not; an empty list releases it.  exits_apply_gradient then gives grad u for any
        Dirichlet colours, exits_adjoint_gradient its derivative with respect to them; exits_apply and exits_adjoint see the
        mean of the walks from the first points.  Returns the stats as a dict"""
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, self._dim)
        return self._dev_solve("exits_walk_gradient", _fp(p), len(p), int(walks), *self._gradient_seeds(len(p), seed_base, walk_seed_base, seed_width))

    def exits_walk_gradient_dev(self, points_ptr, n, walks, stream_ptr=None, seed_base=0, walk_seed_base=None, seed_width=None):
        """the same from a device pointer (int) to n * dim floats on the caller's stream; a point with a non-finite coordinate
        is never walked and answers NaN.  Returns the stats as a dict"""
        return self._dev_solve("exits_walk_gradient_dev", C.c_void_p(points_ptr), int(n), int(walks),
                               *self._gradient_seeds(int(n), seed_base, walk_seed_base, seed_width), C.c_void_p(stream_ptr or 0))

    def exits_gradient_records(self):
        """the gradient part of the list: {"radius" (n,), "dirs" (n, S, dim), "first_pts" (n, S, dim)}, float32"""
        fn, name = self._fn("exits_gradient_records")
        n, S = self.exits_done
        m = max(n * S, 1)      # (with no list bound the call says so; its pointers are still real ones)
        out = {"radius": np.zeros(max(n, 1), np.float32), "dirs": np.zeros(m * self._dim, np.float32), "first_pts": np.zeros(m * self._dim, np.float32)}
        rec = capi.ExitGradientRecords(*[out[k].ctypes.data for k in ("radius", "dirs", "first_pts")])
        _check(fn(self._handle, C.byref(rec)), name)
        return {"radius": out["radius"][:n], "dirs": out["dirs"][:n * S * self._dim].reshape(n, S, self._dim),
                "first_pts": out["first_pts"][:n * S * self._dim].reshape(n, S, self._dim)}

    def exits_apply_gradient(self, colors, want=("stderr", "field")):
        """grad u at the listed points for K sets of Dirichlet colours ([K, n_verts, 6] floats; [n_verts, 6] is one set) -> a dict
        of float32 arrays: "grad" (K, n, dim, 3) and what `want` names of "stderr" (K, n, dim, 3) and "field" (K, n, 3), the
        mean of a point's walks.  With the colours the integrator was made with: solve_gradient_points' outputs, bit for bit"""
        fn, name = self._fn("exits_apply_gradient")
        unknown = set(want) - {"stderr", "field"}
        if unknown:
            raise ValueError("unknown outputs %s (known: stderr, field)" % sorted(unknown))
        c = self._exit_sets(colors, self._exit_verts(), 6)
        K, n = len(c), self.exits_done[0]
        shapes = {"grad": (K, n, self._dim, 3), "stderr": (K, n, self._dim, 3), "field": (K, n, 3)}
        out = {k: np.zeros(shapes[k], np.float32) for k in shapes if k == "grad" or k in want}
        _check(fn(self._handle, _fp(c), K, _fp(out["grad"]), *[_fp(out[k]) if k in out else None for k in ("stderr", "field")]), name)
        return out

    def exits_apply_gradient_dev(self, colors_ptr, K, grad_ptr, stream_ptr=None, stderr_ptr=None, field_ptr=None):
        """the same on device pointers (ints) on the caller's stream: K * n_verts * 6 floats of colours, K * n * dim * 3 of grad
        and, where given, of stderr, K * n * 3 of field"""
        fn, name = self._fn("exits_apply_gradient_dev")
        _check(fn(self._handle, C.c_void_p(colors_ptr), int(K), C.c_void_p(grad_ptr), C.c_void_p(stderr_ptr or 0), C.c_void_p(field_ptr or 0),
                  C.c_void_p(stream_ptr or 0)), name)

    def exits_gradient_terms(self):
        """the in-ball term a list of the gradient carries when it was walked on a scene with a source term under
        set_option("exits_grad_source", 1) (wost_exits_gradient_terms; include/wost.h "Exit lists of the gradient", item 4):
        (T, seT, U), float64 arrays shaped (n, dim, 3), (n, dim, 3) and (n, 3), as exits_apply_gradient joins them to every set of
        colours; zeros at a degenerate point.  Any other list is refused"""
        fn, name = self._fn("exits_gradient_terms")
        n = self.exits_done[0]
        T, seT, U = np.zeros((max(n, 1), self._dim, 3)), np.zeros((max(n, 1), self._dim, 3)), np.zeros((max(n, 1), 3))
        _check(fn(self._handle, *[a.ctypes.data_as(C.POINTER(C.c_double)) for a in (T, seT, U)]), name)
        return T[:n], seT[:n], U[:n]

    def exits_adjoint_gradient(self, dgrad):
        """the transposed map of exits_apply_gradient's grad: dgrad ([K, n, dim, 3] floats; [n, dim, 3] is one set) -> the
        derivative of sum(grad * dgrad) by the colours, (K, n_verts, 6) float32"""
        fn, name = self._fn("exits_adjoint_gradient")
        n = self.exits_done[0]
        d = np.ascontiguousarray(dgrad, dtype=np.float32)
        if d.ndim == 3:
            d = d[None]
        if d.ndim != 4 or d.shape[1:] != (n, self._dim, 3) or len(d) < 1:
            raise ValueError("expected [K, %d, %d, 3] floats, got %s" % (n, self._dim, d.shape))
        out = np.zeros((len(d), self._exit_verts(), 6), np.float32)
        _check(fn(self._handle, _fp(d), len(d), _fp(out)), name)
        return out

    def exits_adjoint_gradient_dev(self, dgrad_ptr, K, dcolors_ptr, stream_ptr=None):
        """the same on device pointers (ints) on the caller's stream: K * n * dim * 3 floats in, K * n_verts * 6 floats out"""
        fn, name = self._fn("exits_adjoint_gradient_dev")
        _check(fn(self._handle, C.c_void_p(dgrad_ptr), int(K), C.c_void_p(dcolors_ptr), C.c_void_p(stream_ptr or 0)), name)

    # -- the index of the exit list and the ordered adjoints (wost_exits_index & co.) -------------
    def exits_index(self):
        """index the bound exit list by vertex (wost_exits_index; include/wost.h "Exit lists: the index and the ordered
        adjoint"), once per walk of the list: the ordered adjoints gather over it.  A second call is a no-op; whatever replaces
        or releases the list drops the index"""
        fn, name = self._fn("exits_index")
        _check(fn(self._handle), name)

    @property
    def exits_index_info(self):
        """(incidences of the index, entries of its longest bin); (0, 0): no index stands"""
        fn, name = self._fn("exits_index_info")
        n_inc, longest = C.c_int64(0), C.c_int64(0)
        _check(fn(self._handle, C.byref(n_inc), C.byref(longest)), name)
        return n_inc.value, longest.value

    def exits_index_records(self):
        """the index: {"bin_begin" (2 n_verts + 1,) int64, "inc" (n_incidences,) int32}; bin 2 v + (side < 0) holds the
        incidences w * dim + j at bin_begin[b] .. bin_begin[b + 1], ascending"""
        fn, name = self._fn("exits_index_records")
        begin = np.zeros(2 * self._exit_verts() + 1, np.int64)
        inc = np.zeros(max(self.exits_index_info[0], 1), np.int32)      # (with no index the call says so; its pointers are still real ones)
        _check(fn(self._handle, begin.ctypes.data_as(C.POINTER(C.c_int64)), capi._ip(inc)), name)
        return {"bin_begin": begin, "inc": inc[:self.exits_index_info[0]]}

    def exits_adjoint_ordered(self, dfield):
        """exits_adjoint as a gather over the index, in a stated summation order: the same bits on every run and every stream"""
        fn, name = self._fn("exits_adjoint_ordered")
        d = self._exit_sets(dfield, self.exits_done[0], 3)
        out = np.zeros((len(d), self._exit_verts(), 6), np.float32)
        _check(fn(self._handle, _fp(d), len(d), _fp(out)), name)
        return out

    def exits_adjoint_ordered_dev(self, dfield_ptr, K, dcolors_ptr, stream_ptr=None):
        """the same on device pointers (ints) on the caller's stream: K * n * 3 floats in, K * n_verts * 6 floats out"""
        fn, name = self._fn("exits_adjoint_ordered_dev")
        _check(fn(self._handle, C.c_void_p(dfield_ptr), int(K), C.c_void_p(dcolors_ptr), C.c_void_p(stream_ptr or 0)), name)

    def exits_adjoint_gradient_ordered(self, dgrad):
        """exits_adjoint_gradient as a gather over the index, in a stated summation order: the same bits on every run"""
        fn, name = self._fn("exits_adjoint_gradient_ordered")
        n = self.exits_done[0]
        d = np.ascontiguousarray(dgrad, dtype=np.float32)
        if d.ndim == 3:
            d = d[None]
        if d.ndim != 4 or d.shape[1:] != (n, self._dim, 3) or len(d) < 1:
            raise ValueError("expected [K, %d, %d, 3] floats, got %s" % (n, self._dim, d.shape))
        out = np.zeros((len(d), self._exit_verts(), 6), np.float32)
        _check(fn(self._handle, _fp(d), len(d), _fp(out)), name)
        return out

    def exits_adjoint_gradient_ordered_dev(self, dgrad_ptr, K, dcolors_ptr, stream_ptr=None):
        """the same on device pointers (ints) on the caller's stream: K * n * dim * 3 floats in, K * n_verts * 6 floats out"""
        fn, name = self._fn("exits_adjoint_gradient_ordered_dev")
        _check(fn(self._handle, C.c_void_p(dgrad_ptr), int(K), C.c_void_p(dcolors_ptr), C.c_void_p(stream_ptr or 0)), name)

    # -- the continued frame solve (wost_solve_more & co.) ---------------------------------------
    def solve_more(self, more_spp):
        """more_spp samples per pixel on top of the carried frame solve; the field of all samples so far -- the solve()'s at
        spp = spp_done, bit for bit -- is in self.solution; returns wall milliseconds"""
        self.solution, st = self._host_solve("solve_more", self.n_pixels, int(more_spp))
        return int(st.solve_ms)

    def solve_more_sharded(self, shard_index, shard_count, more_spp, field_dev_ptr, stream_ptr=None):
        """the same for one shard (as solve_sharded): the carried solve belongs to the shard of its first call"""
        return self._dev_solve("solve_more_sharded", shard_index, shard_count, int(more_spp), C.c_void_p(field_dev_ptr), C.c_void_p(stream_ptr or 0))

    def restart(self):
        """forget the carried solve: spp_done = 0, no shard"""
        fn, name = self._fn("solve_restart")
        _check(fn(self._handle), name)

    @property
    def spp_done(self):
        """samples per pixel of the carried solve so far"""
        fn, name = self._fn("solve_progress")
        n = C.c_int32(0)
        _check(fn(self._handle, C.byref(n)), name)
        return n.value

    def solve_more_where(self, more_spp, select=None):
        """more_spp samples on the pixels whose entry in select (n_pixels values, nonzero = continue) is set; None: every
        pixel, which is solve_more.  Every pixel's field at its own count is in self.solution; returns wall milliseconds"""
        sel = None
        if select is not None:
            sel = np.ascontiguousarray(np.asarray(select).reshape(-1) != 0, dtype=np.uint8)
            if sel.size != self.n_pixels:
                raise ValueError("select has %d entries, the frame %d pixels" % (sel.size, self.n_pixels))
        ptr = sel.ctypes.data_as(C.POINTER(C.c_uint8)) if sel is not None else None
        self.solution, st = self._host_solve("solve_more_where", self.n_pixels, int(more_spp), ptr)
        return int(st.solve_ms)

    def solve_more_where_sharded(self, shard_index, shard_count, more_spp, select_dev_ptr, field_dev_ptr, stream_ptr=None):
        """the same for one shard on device pointers (ints): n_pixels bytes of selection (0: every pixel), a zero-filled field"""
        return self._dev_solve("solve_more_where_sharded", shard_index, shard_count, int(more_spp), C.c_void_p(select_dev_ptr or 0),
                               C.c_void_p(field_dev_ptr), C.c_void_p(stream_ptr or 0))

    def carried(self):
        """the per-pixel state of the carried solve: {"spp": samples done, "batches": calls that walked the pixel, "sum": the
        raw sums (n, 3), "stderr": the batch-means standard error of sum / spp (n, 3), +inf below two batches}"""
        fn, name = self._fn("solve_carried")
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
        fn, name = self._fn("solve_adaptive")
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
        a = self._adaptive(batch_spp, max_spp, abs_tol, rel_tol, min_batches)
        return self._dev_solve("solve_adaptive_sharded", shard_index, shard_count, C.byref(a), C.c_void_p(field_dev_ptr), C.c_void_p(stream_ptr or 0))

    # -- the carried point list (wost_points_carry & co.) ------------------------------------------
    def points_carry(self, points, seed_base=0, seed_width=None):
        """bind a list of evaluation points ([n, dim] floats) to the integrator: the library copies them; point i runs on the
        random stream of pixel seed_base + i in a frame seed_width wide (default: the frame's width), as in solve_points.  The
        list replaces the one bound before, state included; an empty list releases it."""
        fn, name = self._fn("points_carry")
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, self._dim)
        _check(fn(self._handle, _fp(p), len(p), int(seed_base), self._seed_width(seed_width)), name)

    def points_carry_dev(self, points_ptr, n, stream_ptr=None, seed_base=0, seed_width=None):
        """the same from a device pointer (int) to n * dim floats, copied on the caller's stream; a point with a non-finite
        coordinate is never walked and answers NaN"""
        fn, name = self._fn("points_carry_dev")
        _check(fn(self._handle, C.c_void_p(points_ptr), int(n), int(seed_base), self._seed_width(seed_width), C.c_void_p(stream_ptr or 0)), name)

    def _points_progress(self):
        fn, name = self._fn("points_progress")
        n, done = C.c_int32(0), C.c_int32(0)
        _check(fn(self._handle, C.byref(n), C.byref(done)), name)
        return n.value, done.value

    @property
    def n_points(self):
        """points of the bound list (0: none is bound)"""
        return self._points_progress()[0]

    @property
    def points_done(self):
        """the sum of more_spp over the calls on the list since it was bound or restarted"""
        return self._points_progress()[1]

    def points_more(self, more_spp, select=None):
        """more_spp samples on the listed points whose entry in select (n values, nonzero = continue) is set; None: every
        point.  Returns the (n, 3) field: every point's mean at its own count, solve_points' at that spp bit for bit"""
        n = self.n_points
        sel = None
        if select is not None:
            sel = np.ascontiguousarray(np.asarray(select).reshape(-1) != 0, dtype=np.uint8)
            if sel.size != n:
                raise ValueError("select has %d entries, the list %d points" % (sel.size, n))
        ptr = sel.ctypes.data_as(C.POINTER(C.c_uint8)) if sel is not None else None
        return self._host_solve("points_more", n, int(more_spp), ptr)[0]

    def points_more_dev(self, more_spp, field_dev_ptr, select_dev_ptr=None, stream_ptr=None):
        """the same on device pointers (ints): n bytes of selection (None: every point), n * 3 floats of field"""
        return self._dev_solve("points_more_dev", int(more_spp), C.c_void_p(select_dev_ptr or 0), C.c_void_p(field_dev_ptr), C.c_void_p(stream_ptr or 0))

    def points_carried(self):
        """the per-point state of the list, with the keys of carried(): "spp", "batches", "sum", "stderr" """
        fn, name = self._fn("points_carried")
        n = self.n_points
        out = {"spp": np.zeros(n, np.int32), "batches": np.zeros(n, np.int32),
               "sum": np.zeros((n, 3), np.float32), "stderr": np.zeros((n, 3), np.float32)}
        _check(fn(self._handle, _ip(out["spp"]), _ip(out["batches"]), _fp(out["sum"]), _fp(out["stderr"])), name)
        return out

    def points_adaptive(self, batch_spp, max_spp, abs_tol=0.0, rel_tol=0.0, min_batches=4):
        """solve_adaptive over the listed points, from the list's state as it stands; returns (field, stderr, spp): (n, 3),
        (n, 3) and n entries"""
        fn, name = self._fn("points_adaptive")
        n = self.n_points
        field = np.zeros((n, 3), dtype=np.float32)
        se = np.zeros((n, 3), dtype=np.float32)
        spp = np.zeros(n, dtype=np.int32)
        st = Stats()
        a = self._adaptive(batch_spp, max_spp, abs_tol, rel_tol, min_batches)
        _check(fn(self._handle, C.byref(a), _fp(field), _fp(se), _ip(spp), C.byref(st)), name)
        self.last_stats = st.as_dict()
        return field, se, spp

    def points_adaptive_dev(self, batch_spp, max_spp, field_dev_ptr, stream_ptr=None, abs_tol=0.0, rel_tol=0.0, min_batches=4):
        """the same into a device field of n * 3 floats on the caller's stream"""
        a = self._adaptive(batch_spp, max_spp, abs_tol, rel_tol, min_batches)
        return self._dev_solve("points_adaptive_dev", C.byref(a), C.c_void_p(field_dev_ptr), C.c_void_p(stream_ptr or 0))

    def points_restart(self):
        """keep the list, forget its samples"""
        fn, name = self._fn("points_restart")
        _check(fn(self._handle), name)

    # -- lbvh query call sites, batched ---------------------------------------------------------
    def closest_point(self, pts, which=capi.MESH_DIRICHLET):
        fn, name = self._fn("closest_point")
        p = self._points(pts)
        n = len(p)
        idx, dist, side = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.int32)
        uv = np.zeros(n if self._dim == 2 else (n, 2), np.float32)      # a segment's parameter / a triangle's barycentrics
        _check(fn(self._handle, which, _fp(p), n, _ip(idx), _fp(dist), _fp(uv), _ip(side)), name)
        return idx, dist, uv, side

    def closest_silhouette(self, pts, rmax=None, which=capi.MESH_NEUMANN):
        fn, name = self._fn("closest_silhouette")
        p = self._points(pts)
        out = np.zeros(len(p), np.float32)
        r = None if rmax is None else np.ascontiguousarray(rmax, dtype=np.float32)
        _check(fn(self._handle, which, _fp(p), _fp(r) if r is not None else None, len(p), _fp(out)), name)
        return out

    def ray_intersect(self, origins, dirs, tmax, which=capi.MESH_NEUMANN):
        fn, name = self._fn("ray_intersect")
        o, d = self._points(origins), self._points(dirs)
        t = np.ascontiguousarray(tmax, dtype=np.float32)
        n = len(o)
        hit, tt, idx = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.int32)
        _check(fn(self._handle, which, _fp(o), _fp(d), _fp(t), n, _ip(hit), _fp(tt), _ip(idx)), name)
        return hit, tt, idx

    def queryNetwork(self, p):
        raise NotImplementedError("uniform integrator has no network (reference integrator.cu:661-664)")

    def close(self):
        if self._handle:
            self._fn("destroy")[0](self._handle)
            self._handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
