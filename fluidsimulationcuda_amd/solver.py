"""Host-side mirror of the reference's step interface on top of the C ABI.

The reference (project/sequential/FluidSequential.c) exposes its hot path as
plain functions on six (N+2)^2 float arrays: set_bnd, add_source, diffuse,
advect, computeDivergenceAndPressure, lastProject, dens_step, vel_step
(:62-241).  FluidSolver keeps the same names, argument order and meaning, with
the arrays resident on the MI355X and addressed by name.
"""
import ctypes as C
import sys

import numpy as np

from . import capi

# the reference's harness constants (FluidSequential.c:7-9,91)
DT, VIS, DIFF, ITERS = 0.016, 0.0025, 0.1, 40

_ID = {name: k for k, name in enumerate(capi.FIELD_NAMES)}


def _fid(f):
    if isinstance(f, str):
        return _ID[f]
    return int(f)


def _ofid(f):
    """The field of an observing call: a name or id, or None / "point" for capi.FIELD_OF_POINT -- every point of a typed
    network observes its own field."""
    if f is None or f == "point":
        return capi.FIELD_OF_POINT
    return _fid(f)


def _host(a, n):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.shape != (n + 2, n + 2):
        raise ValueError("field must have shape (%d, %d), got %s" % (n + 2, n + 2, a.shape))
    return a


def member_values(members, **params):
    """Scalars or one value per ensemble member, for the physical parameters of a call (dt, diff, visc, alpha, beta).

    All scalars: returns None -- the caller uses the scalar entry point, as ever.  Otherwise every parameter is
    broadcast to a C-contiguous float32 array of length `members` (a dict in the order given), for the `_members`
    entry point.  A sequence of any other length raises ValueError; nothing here touches the library."""
    if all(np.ndim(v) == 0 for v in params.values()):
        return None
    out = {}
    for name, v in params.items():
        a = np.asarray(v, dtype=np.float32)
        if a.ndim == 0:
            a = np.full(members, a, dtype=np.float32)
        elif a.ndim != 1 or a.shape[0] != members:
            raise ValueError("%s: expected a scalar or %d values (one per member), got shape %s" % (name, members, a.shape))
        out[name] = np.ascontiguousarray(a, dtype=np.float32)
    return out


def _mf(a):
    return a.ctypes.data_as(capi._MF)


def device_address(buf):
    """The device address of a buffer: anything with data_ptr() (a torch tensor), a __cuda_array_interface__, or a plain
    integer address."""
    if hasattr(buf, "data_ptr"):
        return int(buf.data_ptr())
    cai = getattr(buf, "__cuda_array_interface__", None)
    if cai is not None:
        return int(cai["data"][0])
    if isinstance(buf, (int, np.integer)):
        return int(buf)
    raise TypeError("a device buffer needs data_ptr(), a __cuda_array_interface__ or an integer address, got %s" % type(buf).__name__)


def device_floats(buf, default):
    """How many floats lie behind a device buffer, where it says so (a plain address: `default`, the caller vouches)."""
    if hasattr(buf, "numel") and hasattr(buf, "element_size"):
        return int(buf.numel()) * int(buf.element_size()) // 4
    cai = getattr(buf, "__cuda_array_interface__", None)
    if cai is not None:
        return int(np.prod(cai["shape"], dtype=np.int64)) * np.dtype(cai["typestr"]).itemsize // 4
    return int(default)


class FluidSolver:
    """Six resident fields + scratch on one GPU (or one row slab of several).

    `members=M` makes it an ensemble: M independent simulations of the same size that go through every call together, in
    the same kernel launches.  Member m's fields are moved with upload(member=m, ...) / download(field, member=m), or all
    at once as (M, N+2, N+2) arrays with upload_members / download_members.  dt, diff, visc (alpha, beta) of step,
    vel_step, dens_step, add_source, diffuse, jacobi_sweep and advect take a scalar for everybody or a sequence with
    one value per member (a parameter study): same launches either way."""

    def __init__(self, n, rank=0, nranks=1, halo=0, jacobi=capi.JACOBI_TB, stream=None,
                 arena_ptr=None, arena_bytes=0, params=None, storage=capi.STORAGE_F32, members=1):
        self._h = C.c_void_p()
        self.n = int(n)
        self.members = int(members)
        self.storage = storage
        cfg = capi.Config(n=self.n, rank=rank, nranks=nranks, halo=halo, jacobi_variant=jacobi,
                          stream=stream, arena=arena_ptr, arena_bytes=arena_bytes, storage=storage)
        if self.members == 1:
            capi.check(capi.lib().fluid_create_ex(C.byref(cfg), C.byref(self._h)))
        else:
            capi.check(capi.lib().fluid_create_ensemble(C.byref(cfg), self.members, C.byref(self._h)))
        lo, hi = C.c_int(), C.c_int()
        capi.check(capi.lib().fluid_owned_rows(self._h, C.byref(lo), C.byref(hi)))
        self.owned_rows = (lo.value, hi.value)
        self.rank, self.nranks = rank, nranks
        self._cb = None
        for key, value in (params or {}).items():     # capi.PARAM_* tuning knobs
            self.set_param(key, value)

    # -- lifetime
    def close(self):
        if self._h:
            capi.lib().fluid_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- data movement
    def upload(self, member=None, **fields):
        """upload(u=..., dens=...) on a single simulation; upload(member=m, u=...) into member m of an ensemble."""
        for name, arr in fields.items():
            if member is None:
                capi.check(capi.lib().fluid_upload(self._h, _fid(name), _host(arr, self.n)))
            else:
                capi.check(capi.lib().fluid_upload_member(self._h, int(member), _fid(name), _host(arr, self.n)))

    def upload_members(self, **fields):
        """Every member of each named field at once: arrays of shape (members, N+2, N+2)."""
        for name, arr in fields.items():
            arr = np.ascontiguousarray(arr, dtype=np.float32)
            if arr.shape != (self.members, self.n + 2, self.n + 2):
                raise ValueError("field must have shape (%d, %d, %d), got %s" % (self.members, self.n + 2, self.n + 2, arr.shape))
            capi.check(capi.lib().fluid_upload_members(self._h, _fid(name), _mf(arr)))

    def download_members(self, field, out=None, coarse=None):
        """All members of a field as one (members, N+2, N+2) array; coarse=r: block-averaged over r x r cells, a
        (members, C, C) array with C = coarse_size(N, r)."""
        side = self.n + 2 if coarse is None else coarse_size(self.n, coarse)
        if out is None:
            out = np.empty((self.members, side, side), dtype=np.float32)
        if out.dtype != np.float32 or not out.flags.c_contiguous or out.shape != (self.members, side, side):
            raise ValueError("out must be C-contiguous float32 of shape (%d, %d, %d)" % (self.members, side, side))
        if coarse is None:
            capi.check(capi.lib().fluid_download_members(self._h, _fid(field), _mf(out)))
        else:
            capi.check(capi.lib().fluid_download_members_coarse(self._h, _fid(field), int(coarse), _mf(out)))
        return out

    # -- whole ensembles on the device: dense float arrays, member after member, each (N+2, N+2) with its ghost ring
    def _handover(self, wait):
        """wait=True: everything torch's current stream holds is done before the library enqueues (a no-op without torch
        or without a device buffer made by it)."""
        if wait:
            torch = sys.modules.get("torch")
            if torch is not None and torch.cuda.is_available():
                torch.cuda.current_stream().synchronize()

    def pack(self, field, out=None, first=0, count=0, member_stride=0, wait=True, coarse=None):
        """Members [first, first + count) of a field (count=0: to the end) into a dense device array, in one launch.

        `out`: a device buffer -- anything with data_ptr(), a __cuda_array_interface__, or an integer address; None: a
        (count, N+2, N+2) float32 torch tensor is allocated (member_stride must then be 0).  wait=True makes the hand-over
        safe both ways: torch's current stream is waited for before the launch is enqueued, the context's stream after
        it.  wait=False only enqueues: for a caller who shares a stream with the library (the constructor's stream=).
        coarse=r (1, 2, 4 .. 64, a divisor of N+2): every r x r block of a member's array as its mean, in the summation
        order the header defines -- a member is then C x C floats, C = coarse_size(N, r), and so is what member_stride
        counts and what is allocated."""
        w = self.n + 2 if coarse is None else coarse_size(self.n, coarse)
        n = int(count) if count else self.members - int(first)
        if out is None:
            if member_stride not in (0, w * w):
                raise ValueError("out=None allocates a dense tensor: member_stride must be 0")
            import torch
            out = torch.empty((max(n, 0), w, w), dtype=torch.float32, device="cuda")
        self._handover(wait)
        if coarse is None:
            capi.check(capi.lib().fluid_pack_members(self._h, _fid(field), int(first), int(count), device_address(out), int(member_stride)))
        else:
            capi.check(capi.lib().fluid_pack_members_coarse(self._h, _fid(field), int(first), int(count), int(coarse), device_address(out),
                                                            int(member_stride)))
        if wait:
            self.synchronize()
        return out

    def unpack(self, field, src, first=0, count=0, member_stride=0, wait=True):
        """A dense device array into members [first, first + count) of a field, in one launch: all members replace the
        field, a sub-range settles it first and overwrites those members.  `src`, `wait`: as for pack."""
        self._handover(wait)
        capi.check(capi.lib().fluid_unpack_members(self._h, _fid(field), int(first), int(count), device_address(src), int(member_stride)))
        if wait:
            self.synchronize()

    # -- recombining an ensemble in place: every new member a linear combination of the old ones
    def transform(self, weights, fields=("u", "v", "dens")):
        """X' = X T per cell of each listed field, in place, one launch per field and no wait: weights[k][m] is the weight
        of OLD member k in NEW member m -- anything np.asarray(.., np.float32) turns into a (members, members) array.  The
        sum runs over the non-zero weights in member order, in double, rounded once (include/fluid_amd.h, "recombining
        ensembles").  members <= capi.TRANSFORM_MAX_MEMBERS."""
        w = np.ascontiguousarray(np.asarray(weights, np.float32))
        if w.shape != (self.members, self.members):
            raise ValueError("weights must have shape (%d, %d), got %s" % (self.members, self.members, w.shape))
        ids = [_fid(f) for f in fields]
        capi.check(capi.lib().fluid_transform_members(self._h, (C.c_int * len(ids))(*ids), len(ids), _mf(w)))

    def select(self, source, fields=("u", "v", "dens")):
        """New member m := old member source[m] in each listed field, in place: branch from one member, resample, permute.
        Bit copies (the transform with the one-hot matrix, in the same launch)."""
        src = [int(s) for s in source]
        if len(src) != self.members:
            raise ValueError("source must name %d members, got %d" % (self.members, len(src)))
        ids = [_fid(f) for f in fields]
        capi.check(capi.lib().fluid_select_members(self._h, (C.c_int * len(ids))(*ids), len(ids), (C.c_int * len(src))(*src)))

    # -- observing an ensemble: a resident network of points, every member's bilinear sample at it, their Gram matrix
    def set_observation_points(self, cols, rows):
        """The observation network: positions in cell-index coordinates (cell centres at 1..N, the walls at 0.5 and
        N + 0.5), two sequences of the same length.  Replaces the previous network; empty sequences clear it
        (include/fluid_amd.h, "observing ensembles")."""
        c = np.ascontiguousarray(np.asarray(cols, np.float32).ravel())
        r = np.ascontiguousarray(np.asarray(rows, np.float32).ravel())
        if c.shape != r.shape:
            raise ValueError("cols and rows must have the same length, got %d and %d" % (c.size, r.size))
        capi.check(capi.lib().fluid_set_observation_points(self._h, _mf(c), _mf(r), int(c.size)))

    def set_observation_network(self, cols, rows, fields=None):
        """set_observation_points with the field each point observes: `fields`, one name or id per point, makes the
        network TYPED -- the observing calls then take field=None (or "point") and read every point from its own field, in
        one call.  fields=None: set_observation_points (include/fluid_amd.h, "typed networks")."""
        if fields is None:
            return self.set_observation_points(cols, rows)
        c = np.ascontiguousarray(np.asarray(cols, np.float32).ravel())
        r = np.ascontiguousarray(np.asarray(rows, np.float32).ravel())
        f = np.ascontiguousarray(np.array([_fid(v) for v in fields], np.int32))
        if not c.size == r.size == f.size:
            raise ValueError("cols, rows and fields must have the same length, got %d, %d and %d" % (c.size, r.size, f.size))
        capi.check(capi.lib().fluid_set_observation_network(self._h, _mf(c), _mf(r), f.ctypes.data_as(C.POINTER(C.c_int)), int(c.size)))

    def observation_fields(self):
        """The names of the fields some point of a typed network observes; empty for an untyped network or none."""
        mask = C.c_uint()
        capi.check(capi.lib().fluid_observation_network_fields(self._h, C.byref(mask)))
        return {name for k, name in enumerate(capi.FIELD_NAMES) if mask.value >> k & 1}

    def observation_points(self):
        """The number of points of the network; 0 when none is set."""
        p = C.c_int()
        capi.check(capi.lib().fluid_observation_points(self._h, C.byref(p)))
        return p.value

    def observe(self, field=None):
        """Every member's value at every point of the network as a (members, points) float32 array: the bilinear sample
        the solver's advection uses, on what pack would show (include/fluid_amd.h, "observing ensembles").  field=None or
        "point", here and in every observing call: each point of a typed network from the field it observes."""
        out = np.empty((self.members, self.observation_points()), np.float32)
        capi.check(capi.lib().fluid_observe_members_host(self._h, _ofid(field), _mf(out)))
        return out

    def observe_device(self, field=None, out=None, member_stride=0, wait=True):
        """observe() into a dense device array, in one launch: out[m * member_stride + p] (member_stride=0: the number of
        points).  `out`, `wait`: as for pack; None: a (members, points) float32 torch tensor is allocated (member_stride
        must then be 0)."""
        if out is None:
            points = self.observation_points()
            if member_stride not in (0, points):
                raise ValueError("out=None allocates a dense tensor: member_stride must be 0")
            import torch
            out = torch.empty((self.members, points), dtype=torch.float32, device="cuda")
        self._handover(wait)
        capi.check(capi.lib().fluid_observe_members(self._h, _ofid(field), device_address(out), int(member_stride)))
        if wait:
            self.synchronize()
        return out

    def observation_gram(self, field=None, obs=None, inv_sigma=None, centre=True):
        """The Gram matrix of the members in observation space: C[k][m] = sum over the points of a_k a_m, a_k = (h_k - mean)
        / sigma (the mean over the members subtracted with `centre`; inv_sigma: 1 / sigma per point, None for 1).  With
        `obs`, the observed values y: returns (C, rhs, dd), rhs[k] = sum a_k d and dd = sum d d for the innovation d =
        (y - mean) / sigma; without: C alone.  Float64, bit-symmetric, the same bits on every call (include/fluid_amd.h,
        "observing ensembles": fluid_observation_gram).  members <= capi.TRANSFORM_MAX_MEMBERS."""
        points = self.observation_points()

        def per_point(a, name):
            if a is None:
                return None
            a = np.ascontiguousarray(np.asarray(a, np.float32).ravel())
            if a.size != points:
                raise ValueError("%s must hold one value per point (%d), got %d" % (name, points, a.size))
            return a

        y, s = per_point(obs, "obs"), per_point(inv_sigma, "inv_sigma")
        dp = C.POINTER(C.c_double)
        g = np.empty((self.members, self.members), np.float64)
        rhs, dd = np.empty(self.members, np.float64), C.c_double()
        capi.check(capi.lib().fluid_observation_gram(self._h, _ofid(field), 1 if centre else 0, None if y is None else _mf(y),
                                                     None if s is None else _mf(s), g.ctypes.data_as(dp),
                                                     None if y is None else rhs.ctypes.data_as(dp), None if y is None else C.byref(dd)))
        return g if y is None else (g, rhs, dd.value)

    def _run_plan(self, nsteps, every, fields, sources, out, iters, use_sources, coarse):
        """The capi.RunPlan of run() and run_window(), and the snapshot array it records into: `out`, a new tensor when it
        is None and something is recorded, None when nothing is."""
        w = self.n + 2 if coarse is None else coarse_size(self.n, coarse)
        ids = [_fid(f) for f in fields]
        every, nsteps = int(every), int(nsteps)
        count = nsteps // every if every > 0 and nsteps > 0 else 0
        capacity = 0
        if every > 0:
            if out is None:
                import torch
                out = torch.empty((count, len(ids), self.members, w, w), dtype=torch.float32, device="cuda")
            capacity = device_floats(out, count * len(ids) * self.members * w * w)
        plan = capi.RunPlan(iters=int(iters), nsteps=nsteps, use_sources=1 if use_sources else 0,
                            sources=device_address(sources) if sources is not None else None, every=every,
                            fields=(C.c_int * len(ids))(*ids) if ids else None, nfields=len(ids),
                            snapshots=device_address(out) if every > 0 else None, capacity=capacity)
        return plan, (out if every > 0 else None)

    def run(self, nsteps, every=0, fields=(), sources=None, out=None, dt=DT, diff=DIFF, visc=VIS, iters=ITERS, use_sources=False,
            wait=True, coarse=None):
        """nsteps steps without the host in the loop.  `sources`: a dense device array (3, members, N+2, N+2) -- u_prev,
        v_prev, dens_prev -- put back before EVERY step (a forced run); None: step()'s rule.  every > 0: after every
        `every`-th step the listed fields are recorded into `out`, a dense device array (snapshots, len(fields), members,
        N+2, N+2) (None: a torch tensor of that shape is allocated).  Returns (out, snapshots written); out is None when
        nothing is recorded.  dt / diff / visc: a scalar or one value per member, like step.  `wait`: as for pack.
        coarse=r: the snapshots are block-averaged like pack(coarse=r), `out` is (snapshots, len(fields), members, C, C);
        the sources stay full resolution."""
        plan, out = self._run_plan(nsteps, every, fields, sources, out, iters, use_sources, coarse)
        written = C.c_int()
        mv = member_values(self.members, dt=dt, diff=diff, visc=visc)
        self._handover(wait)
        tail = (C.byref(plan), C.byref(written)) if coarse is None else (C.byref(plan), int(coarse), C.byref(written))
        name = "fluid_run" if mv is None else "fluid_run_members"
        fn = getattr(capi.lib(), name if coarse is None else name + "_coarse")
        capi.check(fn(self._h, *((dt, diff, visc) if mv is None else [_mf(a) for a in mv.values()]), *tail))
        if wait:
            self.synchronize()
        return out, written.value

    def member_count(self):
        m = C.c_int()
        capi.check(capi.lib().fluid_members(self._h, C.byref(m)))
        return m.value

    def upload_rows(self, field, arr, row_lo, row_hi):
        capi.check(capi.lib().fluid_upload_rows(self._h, _fid(field), _host(arr, self.n), row_lo, row_hi))

    def download(self, field, out=None, member=None):
        if out is None:
            out = np.empty((self.n + 2, self.n + 2), dtype=np.float32)
        if member is None:
            capi.check(capi.lib().fluid_download(self._h, _fid(field), _host(out, self.n)))
        else:
            capi.check(capi.lib().fluid_download_member(self._h, int(member), _fid(field), _host(out, self.n)))
        return out

    def download_rows(self, field, out, row_lo, row_hi):
        capi.check(capi.lib().fluid_download_rows(self._h, _fid(field), out, row_lo, row_hi))
        return out

    def fill(self, field, value=0.0):
        capi.check(capi.lib().fluid_fill(self._h, _fid(field), value))

    def synchronize(self):
        capi.check(capi.lib().fluid_synchronize(self._h))

    def field_ptr(self, field):
        p = C.c_void_p()
        capi.check(capi.lib().fluid_field_ptr(self._h, _fid(field), C.byref(p)))
        return p.value

    def scalar_ptr(self):
        p = C.c_void_p()
        capi.check(capi.lib().fluid_scalar_ptr(self._h, C.byref(p)))
        return p.value

    # -- the reference's operators (same names / argument order)
    def set_bnd(self, b, x):
        capi.check(capi.lib().fluid_op_set_bnd(self._h, b, _fid(x)))

    def _call(self, name, before, params, after=()):
        """fluid_<name>(handle, *before, <params>, *after) when every parameter is a scalar; as soon as one is a sequence,
        fluid_<name>_members with each parameter as an array of one value per member (member_values)"""
        mv = member_values(self.members, **params)
        if mv is None:
            fn, values = getattr(capi.lib(), "fluid_" + name), params.values()
        else:
            fn, values = getattr(capi.lib(), "fluid_" + name + "_members"), [_mf(a) for a in mv.values()]
        capi.check(fn(self._h, *before, *values, *after))

    def add_source(self, x, s, dt=DT):
        self._call("op_add_source", (_fid(x), _fid(s)), dict(dt=dt))

    def jacobi_sweep(self, b, x, x0, out, alpha, beta):
        self._call("op_jacobi_sweep", (b, _fid(x), _fid(x0), _fid(out)), dict(alpha=alpha, beta=beta))

    def diffuse(self, b, x, x0, alpha, beta, iters=ITERS):
        self._call("op_diffuse", (b, _fid(x), _fid(x0)), dict(alpha=alpha, beta=beta), (iters,))

    def advect(self, b, d, d0, u, v, dt=DT):
        self._call("op_advect", (b, _fid(d), _fid(d0), _fid(u), _fid(v)), dict(dt=dt))

    def computeDivergenceAndPressure(self, u, v, p, div):
        capi.check(capi.lib().fluid_op_divergence(self._h, _fid(u), _fid(v), _fid(p), _fid(div)))

    def lastProject(self, u, v, p, div=None):
        capi.check(capi.lib().fluid_op_subtract_gradient(self._h, _fid(u), _fid(v), _fid(p)))

    def vel_step(self, visc=VIS, dt=DT, iters=ITERS):
        """vel_step(u, v, u_prev, v_prev, visc) on the resident fields."""
        self._call("vel_step", (), dict(dt=dt, visc=visc), (iters,))

    def dens_step(self, diff=DIFF, dt=DT, iters=ITERS):
        """dens_step(dens, dens_prev, u, v, diff) on the resident fields."""
        self._call("dens_step", (), dict(dt=dt, diff=diff), (iters,))

    def step(self, nsteps=1, use_sources=False, dt=DT, diff=DIFF, visc=VIS, iters=ITERS):
        """nsteps bodies of the reference's main loop (FluidSequential.c:289-312)."""
        self._call("step", (), dict(dt=dt, diff=diff, visc=visc), (iters, nsteps, 1 if use_sources else 0))

    # -- diagnostics / tuning
    def residual(self, x, x0, alpha, beta):
        out = C.c_float()
        capi.check(capi.lib().fluid_residual(self._h, _fid(x), _fid(x0), alpha, beta, C.byref(out)))
        return out.value

    def absmax_velocity(self, u="u", v="v"):
        out = C.c_float()
        capi.check(capi.lib().fluid_absmax_velocity(self._h, _fid(u), _fid(v), C.byref(out)))
        return out.value

    # -- looking at an ensemble: one value per member, sums per member, statistics across the members
    def residual_members(self, x, x0, alpha, beta):
        """fluid_residual per member, each with its own coefficients (a scalar or one value per member each): a float32
        array of `members` values."""
        mv = member_values(self.members, alpha=alpha, beta=beta)
        if mv is None:      # all scalars: broadcast here, this call always returns one value per member
            mv = {"alpha": np.full(self.members, alpha, np.float32), "beta": np.full(self.members, beta, np.float32)}
        out = np.empty(self.members, np.float32)
        capi.check(capi.lib().fluid_residual_members(self._h, _fid(x), _fid(x0), _mf(mv["alpha"]), _mf(mv["beta"]), _mf(out)))
        return out

    def absmax_velocity_members(self, u="u", v="v"):
        out = np.empty(self.members, np.float32)
        capi.check(capi.lib().fluid_absmax_velocity_members(self._h, _fid(u), _fid(v), _mf(out)))
        return out

    def member_moments(self, field):
        """(sum of x, sum of x*x) over each member's interior cells: two float64 arrays of `members` values."""
        s, q = np.empty(self.members, np.float64), np.empty(self.members, np.float64)
        dp = C.POINTER(C.c_double)
        capi.check(capi.lib().fluid_member_moments(self._h, _fid(field), s.ctypes.data_as(dp), q.ctypes.data_as(dp)))
        return s, q

    def member_gram(self, field, centre=False):
        """The (members, members) float64 matrix of inner products between the members of a field over the interior cells;
        with `centre`, between their anomalies about the per-cell ensemble mean.  Bit-symmetric, the same bits on every
        call (include/fluid_amd.h, "ensemble diagnostics": fluid_member_gram).  members <= capi.TRANSFORM_MAX_MEMBERS."""
        g = np.empty((self.members, self.members), np.float64)
        capi.check(capi.lib().fluid_member_gram(self._h, _fid(field), 1 if centre else 0, g.ctypes.data_as(C.POINTER(C.c_double))))
        return g

    def ensemble_stats(self, field, mean=True, variance=True):
        """Per cell across the members: (mean, population variance) as (N+2, N+2) float32 arrays; None for the one not
        asked for.  With neither, the statistics are only enqueued and stay on the device (ensemble_stats_ptr)."""
        w = self.n + 2
        mu = np.empty((w, w), np.float32) if mean else None
        var = np.empty((w, w), np.float32) if variance else None
        capi.check(capi.lib().fluid_ensemble_stats(self._h, _fid(field), _mf(mu) if mean else None, _mf(var) if variance else None))
        return mu, var

    def ensemble_stats_ptr(self):
        """Device addresses (mean, variance) of the float fields the last ensemble_stats filled (layout of fluid_layout)."""
        mu, var = C.c_void_p(), C.c_void_p()
        capi.check(capi.lib().fluid_ensemble_stats_ptr(self._h, C.byref(mu), C.byref(var)))
        return mu.value, var.value

    # -- localised updates: the increment of a transform under a per-cell taper, over a box of cells
    def transform_local(self, increments, taper=None, box=None, fields=("u", "v", "dens")):
        """X' = X + g o (X D) per cell of each listed field, in place, one launch per field over the box only and no wait:
        increments[k][m] is the weight of OLD member k in the INCREMENT of new member m (D = T - I for a transform T).
        `taper`: a device buffer of (N+2) x (N+2) floats (as pack takes one; taper_gaspari_cohn makes one), None for 1
        everywhere; torch's current stream is waited for before the launch, and the solver keeps the buffer referenced
        until the next call.  `box`: (row_lo, row_hi, col_lo, col_hi), half-open, None for the whole array.  Cells
        outside the box or with taper 0 keep their bits (include/fluid_amd.h, "localised updates").
        members <= capi.TRANSFORM_MAX_MEMBERS."""
        d = np.ascontiguousarray(np.asarray(increments, np.float32))
        if d.shape != (self.members, self.members):
            raise ValueError("increments must have shape (%d, %d), got %s" % (self.members, self.members, d.shape))
        w = self.n + 2
        address = None
        if taper is not None:
            if device_floats(taper, w * w) < w * w:
                raise ValueError("taper must hold (N+2)^2 = %d floats, got %d" % (w * w, device_floats(taper, w * w)))
            address = device_address(taper)
            self._handover(True)
        if box is not None:
            b = [int(v) for v in box]
            if len(b) != 4:
                raise ValueError("box must be (row_lo, row_hi, col_lo, col_hi), got %d values" % len(b))
            box = (C.c_int * 4)(*b)
        ids = [_fid(f) for f in fields]
        capi.check(capi.lib().fluid_transform_members_local(self._h, (C.c_int * len(ids))(*ids), len(ids), _mf(d), address, box))
        self._taper = taper

    def taper_gaspari_cohn(self, col, row, c):
        """The Gaspari-Cohn taper of half-width c (support radius 2c) about (col, row), in the cell-index coordinates of
        set_observation_points: ((N+2, N+2) float32 torch tensor on the device, box) -- the box (row_lo, row_hi, col_lo,
        col_hi) holds every non-zero cell; both are what transform_local takes.  Waits for the context's stream: the tensor
        is complete on return."""
        import torch
        w = self.n + 2
        out = torch.empty((w, w), dtype=torch.float32, device="cuda")
        box = (C.c_int * 4)()
        self._handover(True)
        capi.check(capi.lib().fluid_taper_gaspari_cohn(self._h, float(col), float(row), float(c), device_address(out), box))
        self.synchronize()
        return out, tuple(box)

    # -- lattice updates: increments at the nodes of a coarse lattice, blended bilinearly to every cell
    def transform_lattice(self, increments, origin, step, fields=("u", "v", "dens")):
        """X' = X + sum_b phi_b o (X D_b) per cell of each listed field, every product on the OLD X, in place, one launch
        per field whatever the node count and no wait: increments[a][b][k][m] is the weight of OLD member k in the
        INCREMENT of new member m at node (a, b), shape (nodes_row, nodes_col, members, members); node (a, b) sits on cell
        row origin[0] + a * step, column origin[1] + b * step (any ints), `step` a positive multiple of 8; phi is the
        bilinear weight of the node at the cell, constant outside the lattice's hull (include/fluid_amd.h, "lattice
        updates").  members <= capi.TRANSFORM_MAX_MEMBERS."""
        d = np.ascontiguousarray(np.asarray(increments, np.float32))
        if d.ndim != 4 or d.shape[2:] != (self.members, self.members):
            raise ValueError("increments must have shape (nodes_row, nodes_col, %d, %d), got %s" % (self.members, self.members, d.shape))
        row0, col0 = (int(v) for v in origin)
        ids = [_fid(f) for f in fields]
        capi.check(capi.lib().fluid_transform_members_lattice(self._h, (C.c_int * len(ids))(*ids), len(ids), _mf(d), d.shape[0], d.shape[1],
                                                              row0, col0, int(step)))

    # -- lattice observations: the localised Gram matrix of every node of a lattice, in one call
    def observation_gram_lattice(self, field, shape, origin, step, c, obs=None, inv_sigma=None, centre=True):
        """observation_gram per node of a lattice, every point weighted by the Gaspari-Cohn taper of half-width c about the
        node: C[a][b][k][m] = sum over the points of (w a_k) a_m.  `shape` = (nodes_row, nodes_col), `origin`, `step`: the
        lattice of transform_lattice, so result [a][b] lines up with increments[a][b].  Returns (C, counts), or with `obs`
        (C, rhs, dd, counts): float64 arrays of shape (nr, nc, M, M), (nr, nc, M), (nr, nc) and the int32 number of points
        each node sees, (nr, nc); a node that sees none has zeros.  Every point is observed once, two launches and one wait
        whatever the node count; the same bits on every call (include/fluid_amd.h, "lattice observations")."""
        points = self.observation_points()

        def per_point(a, name):
            if a is None:
                return None
            a = np.ascontiguousarray(np.asarray(a, np.float32).ravel())
            if a.size != points:
                raise ValueError("%s must hold one value per point (%d), got %d" % (name, points, a.size))
            return a

        y, s = per_point(obs, "obs"), per_point(inv_sigma, "inv_sigma")
        nr, nc = (int(v) for v in shape)
        row0, col0 = (int(v) for v in origin)
        m, dp = self.members, C.POINTER(C.c_double)
        room = (max(nr, 0), max(nc, 0))                  # (a refused shape still needs arrays to hand over)
        g = np.empty(room + (m, m), np.float64)
        rhs, dd = np.empty(room + (m,), np.float64), np.empty(room, np.float64)
        counts = np.empty(room, np.int32)
        capi.check(capi.lib().fluid_observation_gram_lattice(
            self._h, _ofid(field), 1 if centre else 0, None if y is None else _mf(y), None if s is None else _mf(s), nr, nc, row0, col0,
            int(step), float(c), g.ctypes.data_as(dp), None if y is None else rhs.ctypes.data_as(dp),
            None if y is None else dd.ctypes.data_as(dp), counts.ctypes.data_as(C.POINTER(C.c_int))))
        return (g, counts) if y is None else (g, rhs, dd, counts)

    # -- one-call analysis: the ETKF solved per node on the device, and Gram -> solve -> lattice update without a wait
    def etkf_increments(self, C_, rhs, counts=None, rho=1.0):
        """The ETKF increment D = W - I + w 1^T of every node from its Gram matrix and right-hand side (what
        observation_gram_lattice returns), S = (M - 1) / rho I + C solved by Jacobi rotations on the device, every node in
        one launch: C_ (..., M, M) and rhs (..., M) float64, counts (...) ints or None, rho the multiplicative inflation.
        Returns (D float32 (..., M, M), status int32 (...)): 0 solved, 1 empty (counts == 0: D = 0), 2 failed (D = 0).
        Only the upper triangle of C_ is read; the same bits for a node whatever the batch (include/fluid_amd.h, "one-call
        analysis")."""
        m, dp = self.members, C.POINTER(C.c_double)
        g = np.ascontiguousarray(np.asarray(C_, np.float64))
        r = np.ascontiguousarray(np.asarray(rhs, np.float64))
        if g.ndim < 2 or g.shape[-2:] != (m, m):
            raise ValueError("C must have shape (..., %d, %d), got %s" % (m, m, g.shape))
        lead = g.shape[:-2]
        if r.shape != lead + (m,):
            raise ValueError("rhs must have shape %s, got %s" % (lead + (m,), r.shape))
        n = None
        if counts is not None:
            n = np.ascontiguousarray(np.asarray(counts, np.int32))
            if n.shape != lead:
                raise ValueError("counts must have shape %s, got %s" % (lead, n.shape))
        nodes = int(np.prod(lead, dtype=np.int64))
        d, status = np.empty(lead + (m, m), np.float32), np.empty(lead, np.int32)
        capi.check(capi.lib().fluid_etkf_increments(self._h, nodes, g.ctypes.data_as(dp), r.ctypes.data_as(dp),
                                                    None if n is None else n.ctypes.data_as(C.POINTER(C.c_int)), float(rho), _mf(d),
                                                    status.ctypes.data_as(C.POINTER(C.c_int))))
        return d, status

    def analyse_lattice(self, field, shape, origin, step, c, obs, inv_sigma=None, rho=1.0, fields=("dens", "u", "v"), wait=True):
        """One assimilation cycle of a localised filter: observation_gram_lattice(field, centre=True), etkf_increments and
        transform_lattice(fields), bit for bit, but chained on the device -- two Gram launches, one solve, one lattice
        launch per listed field; nothing crosses to the host.  `wait=False` returns once everything is enqueued;
        analyse_status() says how the nodes ended (include/fluid_amd.h, "one-call analysis")."""
        points = self.observation_points()

        def per_point(a, name):
            if a is None:
                return None
            a = np.ascontiguousarray(np.asarray(a, np.float32).ravel())
            if a.size != points:
                raise ValueError("%s must hold one value per point (%d), got %d" % (name, points, a.size))
            return a

        y, s = per_point(obs, "obs"), per_point(inv_sigma, "inv_sigma")
        nr, nc = (int(v) for v in shape)
        row0, col0 = (int(v) for v in origin)
        ids = [_fid(f) for f in fields]
        capi.check(capi.lib().fluid_analyse_lattice(self._h, _ofid(field), None if y is None else _mf(y), None if s is None else _mf(s),
                                                    nr, nc, row0, col0, int(step), float(c), float(rho), (C.c_int * len(ids))(*ids),
                                                    len(ids)))
        if wait:
            self.synchronize()

    def analyse_status(self):
        """Waits for the stream; {"solved", "empty", "failed"}: how many nodes of the last analyse_lattice ended in each
        status."""
        n = [C.c_int(), C.c_int(), C.c_int()]
        capi.check(capi.lib().fluid_analyse_lattice_status(self._h, *(C.byref(v) for v in n)))
        return {"solved": n[0].value, "empty": n[1].value, "failed": n[2].value}

    # -- relaxation to prior spread: the per-cell ensemble standard deviation, and the anomalies rescaled towards an earlier one
    def _spread_tensor(self, t, nfields, name):
        """The address of an (nfields, N+2, N+2) float32 device tensor, checked: a wrong shape, type or layout is an error here."""
        import torch
        w = self.n + 2
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch tensor on the device, got %s" % (name, type(t).__name__))
        if t.dtype != torch.float32 or not t.is_cuda:
            raise ValueError("%s must be a float32 tensor on the device, got %s on %s" % (name, t.dtype, t.device))
        if tuple(t.shape) != (nfields, w, w):
            raise ValueError("%s must have shape (%d, %d, %d), got %s" % (name, nfields, w, w, tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous" % name)
        return int(t.data_ptr())

    def spread(self, fields=("u", "v", "dens"), out=None, wait=True):
        """The sample standard deviation over the members, per cell of each listed field (ghost ring included), as an
        (nfields, N+2, N+2) float32 device tensor: sqrt(q / (members - 1)) in double, q the two-pass sum of squares of
        ensemble_stats, on what pack would show.  One launch per field; any members >= 2.  `out`: such a tensor to fill,
        None allocates one; `wait`: as for pack (include/fluid_amd.h, "relaxation to prior spread")."""
        ids = [_fid(f) for f in fields]
        if out is None:
            import torch
            out = torch.empty((len(ids), self.n + 2, self.n + 2), dtype=torch.float32, device="cuda")
        address = self._spread_tensor(out, len(ids), "out")
        self._handover(wait)
        capi.check(capi.lib().fluid_member_spread(self._h, (C.c_int * len(ids))(*ids), len(ids), address, 0))
        if wait:
            self.synchronize()
        return out

    def relax_spread(self, prior, alpha, fields=("u", "v", "dens"), wait=True):
        """Relaxation to prior spread (RTPS), in place, one launch per listed field: every cell's anomalies about the
        ensemble mean are scaled by 1 + alpha * (prior - sd) / sd, sd the cell's spread now and `prior` what spread()
        returned for the same fields before the analysis.  alpha = 0 changes nothing, alpha = 1 restores the prior spread;
        cells without spread keep their bits.  `prior`: an (nfields, N+2, N+2) float32 device tensor, contiguous; `wait`: as
        for pack (include/fluid_amd.h, "relaxation to prior spread")."""
        ids = [_fid(f) for f in fields]
        address = self._spread_tensor(prior, len(ids), "prior")
        self._handover(wait)
        capi.check(capi.lib().fluid_relax_spread(self._h, (C.c_int * len(ids))(*ids), len(ids), address, 0, float(alpha)))
        if wait:
            self.synchronize()

    # -- verifying ensembles: CRPS, RMSE against spread and the rank histogram against a truth field
    def verify(self, truth, fields=("dens",), box=None, fair=False, crps_map=None, out=None, wait=True):
        """Scores the ensemble against `truth`, per listed field over the cells of `box`, in at most two launches per field:
        one row of capi.VERIFY_ROW float64 per field -- the cell count, the sums of e = mean - truth, e * e, the sample
        variance and the CRPS, then the rank histogram (members + 1 bins) -- which verify_scores turns into numbers.
        `truth`: an (nfields, N+2, N+2) float32 device tensor, contiguous; for a twin experiment truth_ctx.pack("dens").
        `box`: (row_lo, row_hi, col_lo, col_hi), half-open, None for the interior.  `fair`: the CRPS's pair term over
        M (M - 1).  `crps_map`: a tensor like `truth` that receives the per-cell CRPS inside the box, None for no map.
        `out`: an (nfields, capi.VERIFY_ROW) float64 device tensor, contiguous -- a row-slice of a larger one will do --, None
        allocates it.  Returns `out`; `wait`: as for pack.  2 <= members <= capi.TRANSFORM_MAX_MEMBERS (include/fluid_amd.h,
        "verifying ensembles")."""
        import torch
        ids = [_fid(f) for f in ((fields,) if isinstance(fields, (str, int)) else fields)]
        address = self._spread_tensor(truth, len(ids), "truth")
        map_address = None if crps_map is None else self._spread_tensor(crps_map, len(ids), "crps_map")
        if out is None:
            out = torch.empty((len(ids), capi.VERIFY_ROW), dtype=torch.float64, device="cuda")
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or not out.is_cuda:
            raise ValueError("out must be a float64 tensor on the device")
        if tuple(out.shape) != (len(ids), capi.VERIFY_ROW) or not out.is_contiguous():
            raise ValueError("out must be contiguous with shape (%d, %d), got %s" % (len(ids), capi.VERIFY_ROW, tuple(out.shape)))
        if box is not None:
            b = [int(v) for v in box]
            if len(b) != 4:
                raise ValueError("box must be (row_lo, row_hi, col_lo, col_hi), got %d values" % len(b))
            box = (C.c_int * 4)(*b)
        self._handover(wait)
        capi.check(capi.lib().fluid_verify_members(self._h, (C.c_int * len(ids))(*ids), len(ids), address, 0, box,
                                                   capi.VERIFY_FAIR if fair else 0, map_address, int(out.data_ptr())))
        if wait:
            self.synchronize()
        return out

    def verify_scores(self, out):
        """What verify left in `out`, after a wait for the context's stream: one dict per field (for a tensor of more
        dimensions, nested lists of them) with `count`, `bias`, `rmse`, `spread`, `crps` and `rank_hist` (int64, members + 1
        entries).  An empty box gives NaN scores."""
        self.synchronize()
        rows = out.cpu().numpy() if hasattr(out, "cpu") else np.asarray(out)
        if rows.ndim > 2:
            return [self.verify_scores(r) for r in rows]
        s = capi.VERIFY_SUMS
        res = []
        with np.errstate(divide="ignore", invalid="ignore"):
            for r in np.atleast_2d(rows):
                n = r[0]
                res.append({"count": int(n), "bias": float(r[1] / n), "rmse": float(np.sqrt(r[2] / n)), "spread": float(np.sqrt(r[3] / n)),
                            "crps": float(r[4] / n), "rank_hist": r[s:s + self.members + 1].astype(np.int64)})
        return res

    # -- ensemble products: order statistics and exceedance probabilities per cell across the members
    def _levels(self, values, name):
        a = np.ascontiguousarray(np.atleast_1d(np.asarray(values, dtype=np.float32)))
        if a.ndim != 1 or not 1 <= a.size <= capi.QUANTILE_MAX_LEVELS:
            raise ValueError("%s: expected 1 to %d values, got shape %s" % (name, capi.QUANTILE_MAX_LEVELS, a.shape))
        return a

    def quantiles(self, field="dens", levels=(0.5,), out=None, wait=True):
        """Quantile fields of one field across the members, in one launch: an (nlevels, N+2, N+2) float32 device tensor, map l
        the `levels[l]` quantile per cell (ghost ring included) of what pack would show, by numpy's default linear
        interpolation between the order statistics -- 0 the minimum, 0.5 the median, 1 the maximum; -0 counts as +0; a
        cell with a non-finite member is NaN.  Up to capi.QUANTILE_MAX_LEVELS levels in [0, 1], in any order; 1 <= members
        <= capi.TRANSFORM_MAX_MEMBERS.  `out`: such a tensor to fill, None allocates one; `wait`: as for pack
        (include/fluid_amd.h, "ensemble products")."""
        lv = self._levels(levels, "levels")
        if out is None:
            import torch
            out = torch.empty((lv.size, self.n + 2, self.n + 2), dtype=torch.float32, device="cuda")
        address = self._spread_tensor(out, lv.size, "out")
        self._handover(wait)
        capi.check(capi.lib().fluid_member_quantiles(self._h, _fid(field), _mf(lv), lv.size, address, 0))
        if wait:
            self.synchronize()
        return out

    def exceedance(self, field, thresholds, below=False, out=None, wait=True):
        """Exceedance probabilities of one field, in one launch: an (nthresholds, N+2, N+2) float32 device tensor, map l the
        fraction of members whose value lies above `thresholds[l]` (`below`: beneath it) per cell of what pack would show.
        A NaN member counts as neither.  Up to capi.QUANTILE_MAX_LEVELS finite thresholds; any members >= 1.  `out`, `wait`:
        as for quantiles (include/fluid_amd.h, "ensemble products")."""
        th = self._levels(thresholds, "thresholds")
        if out is None:
            import torch
            out = torch.empty((th.size, self.n + 2, self.n + 2), dtype=torch.float32, device="cuda")
        address = self._spread_tensor(out, th.size, "out")
        self._handover(wait)
        capi.check(capi.lib().fluid_member_exceedance(self._h, _fid(field), _mf(th), th.size,
                                                      capi.EXCEED_BELOW if below else capi.EXCEED_ABOVE, address, 0))
        if wait:
            self.synchronize()
        return out

    # -- ensemble noise: reproducible randomness on the device, the same bits for every members, launch shape and process
    def _amplitudes(self, amplitude):
        a = np.asarray(amplitude, dtype=np.float32)
        if a.ndim == 0:
            a = np.full(self.members, a, dtype=np.float32)
        elif a.ndim != 1 or a.shape[0] != self.members:
            raise ValueError("amplitude: expected a scalar or %d values (one per member), got shape %s" % (self.members, a.shape))
        return np.ascontiguousarray(a, dtype=np.float32)

    def noise(self, fields, amplitude, seed, sequence=0, mode=capi.NOISE_SET, member_offset=0):
        """Approximately normal noise (mean 0, variance 1, |z| <= 4.899; Philox4x32-10, eight 16-bit halves summed) times
        `amplitude` -- a scalar or one value per member -- set into (mode capi.NOISE_SET or "set") or added to (capi.NOISE_ADD
        or "add") every cell of every member of the listed fields, ghost ring included, in one launch per field, no wait.
        The noise of (seed, sequence, field, member_offset + member, cell) is the same bits whatever `members` is: contexts
        that hold parts of one big ensemble pass the index of their first member as `member_offset`.  A new `sequence` per
        cycle gives new noise under one `seed` (include/fluid_amd.h, "ensemble noise")."""
        ids = [_fid(f) for f in ((fields,) if isinstance(fields, (str, int)) else fields)]
        mode = {"set": capi.NOISE_SET, "add": capi.NOISE_ADD}.get(mode, mode)
        a = self._amplitudes(amplitude)
        capi.check(capi.lib().fluid_noise_members(self._h, (C.c_int * len(ids))(*ids), len(ids), int(mode), _mf(a), int(seed), int(sequence),
                                                  int(member_offset)))

    def noise_dense(self, out, amplitude, seed, sequence=0, stream_id=0, count=None, wait=True):
        """out[q] = amplitude * z for the first `count` floats of a dense device buffer (None: all of it; a plain address
        needs a count), z of the stream `stream_id` in [0, 65535] of (seed, sequence): the observation noise of a twin
        experiment, or the perturbed observations of a stochastic filter.  One launch; `wait`: as for pack.  Returns `out`."""
        if count is None:
            count = device_floats(out, -1)
            if count < 0:
                raise ValueError("noise_dense: a plain address needs a count")
        elif device_floats(out, count) < count:
            raise ValueError("noise_dense: the buffer holds %d floats, count is %d" % (device_floats(out, count), count))
        self._handover(wait)
        capi.check(capi.lib().fluid_noise_dense(self._h, device_address(out), int(count), float(amplitude), int(seed), int(sequence),
                                                int(stream_id)))
        if wait:
            self.synchronize()
        return out

    def perturb(self, field, scratch, amplitude, seed, sequence, alpha, beta, iters, b=0):
        """Spatially correlated noise added to `field`: white noise of amplitude 1 set into scratch[0], smoothed by the
        implicit diffusion solve (Weaver & Courtier 2001) diffuse(b, scratch[1], scratch[0], alpha, beta, iters), and the
        result added as add_source(field, scratch[1], dt=amplitude) -- those three calls and nothing else, so the solve
        starts from what scratch[1] holds.  `scratch`: two of the six fields (the solve's right-hand side and its result),
        distinct from each other and from `field`; alpha, beta, amplitude: a scalar or one value per member.  Smoothing
        shrinks the variance: measure what one call leaves in scratch[1] once, with member_moments, and rescale `amplitude`
        by 1 / its standard deviation."""
        white, smooth = scratch
        mv = member_values(self.members, alpha=alpha, beta=beta)
        if mv is None:
            mv = {"alpha": np.full(self.members, alpha, np.float32), "beta": np.full(self.members, beta, np.float32)}
        self.noise((white,), 1.0, seed, sequence, capi.NOISE_SET)
        capi.check(capi.lib().fluid_op_diffuse_members(self._h, int(b), _fid(smooth), _fid(white), _mf(mv["alpha"]), _mf(mv["beta"]), int(iters)))
        capi.check(capi.lib().fluid_op_add_source_members(self._h, _fid(field), _fid(smooth), _mf(self._amplitudes(amplitude))))

    # -- asynchronous observations: H x recorded during a run, the analysis formed from the record
    def _per_point(self, a, name):
        if a is None:
            return None
        points = self.observation_points()
        a = np.ascontiguousarray(np.asarray(a, np.float32).ravel())
        if a.size != points:
            raise ValueError("%s must hold one value per point (%d), got %d" % (name, points, a.size))
        return a

    def _record(self, record, member_stride):
        """A record to write: `record`, or -- None -- a new (members, points) float32 torch tensor of zeros."""
        if record is None:
            points = self.observation_points()
            if member_stride not in (0, points):
                raise ValueError("record=None allocates a dense tensor: member_stride must be 0")
            import torch
            record = torch.zeros((self.members, points), dtype=torch.float32, device="cuda")
        return record

    def observe_range(self, first, count, out, field=None, member_stride=0, wait=True):
        """observe_device for the points [first, first + count) only: out[m * member_stride + p] for those p, every other
        float of `out` keeps its bits; one launch, count = 0 launches nothing.  `out` is a RECORD: the layout of
        observe_device's array, whole network wide (include/fluid_amd.h, "asynchronous observations").  `wait`: as for
        pack.  Returns `out`."""
        self._handover(wait)
        capi.check(capi.lib().fluid_observe_members_range(self._h, _ofid(field), int(first), int(count), device_address(out),
                                                          int(member_stride)))
        if wait:
            self.synchronize()
        return out

    def run_window(self, nsteps, slot_first, slot_step, record=None, field=None, member_stride=0, every=0, fields=(), sources=None,
                   out=None, dt=DT, diff=DIFF, visc=VIS, iters=ITERS, use_sources=False, wait=True, coarse=None):
        """run() that observes on the way: slot s, the points [slot_first[s], slot_first[s + 1]) of the network, is observed
        into `record` after slot_step[s] steps (0: before the first), behind that step's snapshots -- each an
        observe_range(slot_first[s], slot_first[s + 1] - slot_first[s], record, field, member_stride).  len(slot_first) =
        len(slot_step) + 1 (both empty: the plain run).  record=None: a (members, points) tensor of zeros is allocated, so
        that points in no slot read 0.  The other keywords are run()'s.  Returns (record, out, snapshots written)."""
        first, step = [int(v) for v in slot_first], [int(v) for v in slot_step]
        if (first or step) and len(first) != len(step) + 1:
            raise ValueError("slot_first must hold one more entry than slot_step (%d), got %d" % (len(step), len(first)))
        record = self._record(record, member_stride)
        plan, out = self._run_plan(nsteps, every, fields, sources, out, iters, use_sources, coarse)
        window = capi.ObsWindow(field=_ofid(field), nslots=len(step), slot_first=(C.c_int * len(first))(*first) if step else None,
                                slot_step=(C.c_int * len(step))(*step) if step else None, record_dev=device_address(record),
                                member_stride=int(member_stride))
        written = C.c_int()
        mv = [np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float32), (self.members,))) for v in (dt, diff, visc)]
        self._handover(wait)
        capi.check(capi.lib().fluid_run_window(self._h, *[_mf(a) for a in mv], C.byref(plan), 0 if coarse is None else int(coarse),
                                               C.byref(window), C.byref(written)))
        if wait:
            self.synchronize()
        return record, out, written.value

    def observation_gram_recorded(self, record, obs=None, inv_sigma=None, centre=True, member_stride=0):
        """observation_gram with h_k[p] read from a record, record[k * member_stride + p], instead of sampled: no field is
        settled or read (include/fluid_amd.h, "asynchronous observations").  A record observe_device just wrote gives
        observation_gram's bits.  What torch's current stream still owes the record is waited for first."""
        y, s = self._per_point(obs, "obs"), self._per_point(inv_sigma, "inv_sigma")
        dp = C.POINTER(C.c_double)
        g = np.empty((self.members, self.members), np.float64)
        rhs, dd = np.empty(self.members, np.float64), C.c_double()
        self._handover(True)
        capi.check(capi.lib().fluid_observation_gram_recorded(
            self._h, device_address(record), int(member_stride), 1 if centre else 0, None if y is None else _mf(y),
            None if s is None else _mf(s), g.ctypes.data_as(dp), None if y is None else rhs.ctypes.data_as(dp),
            None if y is None else C.byref(dd)))
        return g if y is None else (g, rhs, dd.value)

    def observation_gram_lattice_recorded(self, record, shape, origin, step, c, obs=None, inv_sigma=None, centre=True, member_stride=0):
        """observation_gram_lattice from a record: the same returns, the same point lists and their cache."""
        y, s = self._per_point(obs, "obs"), self._per_point(inv_sigma, "inv_sigma")
        nr, nc = (int(v) for v in shape)
        row0, col0 = (int(v) for v in origin)
        m, dp = self.members, C.POINTER(C.c_double)
        room = (max(nr, 0), max(nc, 0))                  # (a refused shape still needs arrays to hand over)
        g = np.empty(room + (m, m), np.float64)
        rhs, dd = np.empty(room + (m,), np.float64), np.empty(room, np.float64)
        counts = np.empty(room, np.int32)
        self._handover(True)
        capi.check(capi.lib().fluid_observation_gram_lattice_recorded(
            self._h, device_address(record), int(member_stride), 1 if centre else 0, None if y is None else _mf(y),
            None if s is None else _mf(s), nr, nc, row0, col0, int(step), float(c), g.ctypes.data_as(dp),
            None if y is None else rhs.ctypes.data_as(dp), None if y is None else dd.ctypes.data_as(dp),
            counts.ctypes.data_as(C.POINTER(C.c_int))))
        return (g, counts) if y is None else (g, rhs, dd, counts)

    def analyse_lattice_recorded(self, record, shape, origin, step, c, obs, inv_sigma=None, rho=1.0, fields=("dens", "u", "v"), wait=True,
                                 member_stride=0):
        """analyse_lattice from a record: the weights come from what the members showed when each observation was taken,
        and are applied to `fields` as they are now -- the 4D-LETKF of a window recorded by run_window.  Only `fields` are
        settled and updated; analyse_status() serves this call too."""
        y, s = self._per_point(obs, "obs"), self._per_point(inv_sigma, "inv_sigma")
        nr, nc = (int(v) for v in shape)
        row0, col0 = (int(v) for v in origin)
        ids = [_fid(f) for f in fields]
        self._handover(wait)
        capi.check(capi.lib().fluid_analyse_lattice_recorded(
            self._h, device_address(record), int(member_stride), None if y is None else _mf(y), None if s is None else _mf(s), nr, nc,
            row0, col0, int(step), float(c), float(rho), (C.c_int * len(ids))(*ids), len(ids)))
        if wait:
            self.synchronize()

    # -- screening observations: departures, ranks and the background check, on the device
    def set_observation_qc(self, threshold):
        """The resident background check: while threshold > 0, observation_gram, observation_gram_lattice, analyse_lattice
        and their _recorded namesakes, given `obs`, first reject every point with d^2 > threshold^2 (1 + var / sigma^2) --
        d the normalised departure from the ensemble mean, var the ensemble variance of h -- and proceed as with inv_sigma 0
        there; one more launch, no wait.  0 (the default) is off; the value outlives the network (include/fluid_amd.h,
        "screening observations")."""
        capi.check(capi.lib().fluid_set_observation_qc(self._h, float(threshold)))

    def observation_qc(self):
        """The resident threshold; 0: the gate is off."""
        t = C.c_float()
        capi.check(capi.lib().fluid_observation_qc(self._h, C.byref(t)))
        return t.value

    def observation_qc_result(self):
        """Waits for the stream; (flags, checked, rejected) of the last gated call: a uint8 array with 1 at the rejected
        points, the number of points and the number of flags set."""
        flags = np.empty(self.observation_points(), np.uint8)
        checked, rejected = C.c_int(), C.c_int()
        capi.check(capi.lib().fluid_observation_qc_result(self._h, flags.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(checked),
                                                          C.byref(rejected)))
        return flags, checked.value, rejected.value

    def observation_departures(self, field=None, record=None, obs=None, inv_sigma=None, threshold=0.0, member_stride=0):
        """What observation-space verification needs, per point of the network, in at most two launches and one wait: a
        dict with "mean" and "spread" (float32: the ensemble mean and sample standard deviation of h) and, with `obs`,
        "departure" (float32, y - mean), "rank" (uint8: the members below y, 0 .. M), "flag" (uint8: 1 where the background
        check at `threshold` rejects the point; 0 rejects nothing) and "sums" (float64[3] over the points not rejected:
        their count, the sum of d^2, the sum of var / sigma^2 -- (sums[1] - sums[0]) / sums[2] estimates the inflation the
        ensemble lacks).  `record`: a record to read h from (record[k * member_stride + p]) instead of sampling `field`.
        The resident gate is not touched (include/fluid_amd.h, "screening observations")."""
        y, s = self._per_point(obs, "obs"), self._per_point(inv_sigma, "inv_sigma")
        points = self.observation_points()
        bp, dp = C.POINTER(C.c_ubyte), C.POINTER(C.c_double)
        out = {"mean": np.empty(points, np.float32), "spread": np.empty(points, np.float32)}
        if y is not None:
            out.update(departure=np.empty(points, np.float32), rank=np.empty(points, np.uint8), flag=np.empty(points, np.uint8),
                       sums=np.empty(3, np.float64))
        tail = [None if y is None else _mf(y), None if s is None else _mf(s), float(threshold), _mf(out["mean"]), _mf(out["spread"]),
                None if y is None else _mf(out["departure"]), None if y is None else out["rank"].ctypes.data_as(bp),
                None if y is None else out["flag"].ctypes.data_as(bp), None if y is None else out["sums"].ctypes.data_as(dp)]
        if record is None:
            capi.check(capi.lib().fluid_observation_departures(self._h, _ofid(field), *tail))
        else:
            self._handover(True)
            capi.check(capi.lib().fluid_observation_departures_recorded(self._h, device_address(record), int(member_stride), *tail))
        return out

    def set_jacobi_variant(self, variant):
        capi.check(capi.lib().fluid_set_jacobi_variant(self._h, variant))

    def division_mode(self, alpha, beta):
        """0 true division, 2 double reciprocal, 3 two-term reciprocal (tile-proved), 4 exact reciprocal,
        5 float reciprocal + scaled residual correction."""
        m = C.c_int()
        capi.check(capi.lib().fluid_division_mode(self._h, alpha, beta, C.byref(m)))
        return m.value

    def autotune_pending(self):
        """Launch shapes whose strip height the run-time tuner is still measuring (process-wide)."""
        m = C.c_int()
        capi.check(capi.lib().fluid_autotune_pending(self._h, C.byref(m)))
        return m.value

    def set_param(self, key, value):
        capi.check(capi.lib().fluid_set_param(self._h, key, value))

    def timing_enable(self, on=True):
        capi.check(capi.lib().fluid_timing_enable(self._h, 1 if on else 0))

    def timing_read(self, reset=True):
        t = capi.Timing()
        capi.check(capi.lib().fluid_timing_read(self._h, C.byref(t), 1 if reset else 0))
        out = {"jacobi_ms": t.jacobi_ms, "sweeps": t.sweeps, "solves": t.solves,
               "jacobi_launches": t.jacobi_launches, "jacobi_field_launches": t.jacobi_field_launches,
               "pressure_ms": t.pressure_ms, "pressure_sweeps": t.pressure_sweeps}
        for k, name in enumerate(capi.TIMING_CATEGORIES):
            out[name + "_ms"] = t.category_ms[k]
            out[name + "_calls"] = t.category_calls[k]
        return out

    def diffuse_tol(self, b, x, x0, alpha, beta, tol, max_iters=10000, check_every=8):
        """Opt-in, not the reference's behaviour: sweep until the residual <= tol.
        Returns (sweeps done, final residual)."""
        it, res = C.c_int(), C.c_float()
        capi.check(capi.lib().fluid_op_diffuse_tol(self._h, b, _fid(x), _fid(x0), alpha, beta, tol, max_iters,
                                                   check_every, C.byref(it), C.byref(res)))
        return it.value, res.value

    def split_launches(self):
        """Jacobi launches that ran as interior + edge strips around an exchange in flight (row slabs)."""
        m = C.c_longlong()
        capi.check(capi.lib().fluid_split_launches(self._h, C.byref(m)))
        return m.value

    def exchange_stream(self):
        """hipStream_t (as an integer) an exchange callback should enqueue on right now."""
        p = C.c_void_p()
        capi.check(capi.lib().fluid_exchange_stream(self._h, C.byref(p)))
        return p.value or 0

    def set_exchange(self, fn):
        """fn(kind, fields, depth, scalar_or_None) -> new scalar or None; raises on failure."""
        if fn is None:
            self._cb = None
            capi.check(capi.lib().fluid_set_exchange(self._h, C.cast(None, capi.EXCHANGE_FN), None))
            return

        def tramp(_user, kind, fields, nfields, depth, scalar):
            try:
                ids = [fields[k] for k in range(nfields)]
                if kind in (capi.XCHG_MAX, capi.XCHG_MAX_END):
                    scalar[0] = float(fn(kind, ids, depth, float(scalar[0])))
                else:
                    fn(kind, ids, depth, None)
                return 0
            except Exception:  # never let an exception cross the C boundary
                import traceback
                traceback.print_exc()
                return 1

        self._cb = capi.EXCHANGE_FN(tramp)
        capi.check(capi.lib().fluid_set_exchange(self._h, self._cb, None))


def coarse_size(n, factor):
    """Side C = (n + 2) / factor of a block-averaged member; raises FluidError unless factor is one of 1, 2, 4 .. 64 and
    divides n + 2 (fluid_coarse_size: host logic, no device)."""
    side = C.c_int()
    capi.check(capi.lib().fluid_coarse_size(int(n), int(factor), C.byref(side)))
    return side.value


def noise_value(seed, sequence, tag, member_id, c0, c1):
    """The z of one counter of the ensemble noise: (c0, c1, (tag << 16) | member_id, sequence) under `seed` -- for a field
    cell tag = the field id, c0 = the column, c1 = the row (fluid_noise_value: host logic, no device)."""
    z = C.c_double()
    capi.check(capi.lib().fluid_noise_value(int(seed), int(sequence), int(tag), int(member_id), int(c0), int(c1), C.byref(z)))
    return z.value


def quantile_position(members, level):
    """(lo, frac): where the `level` quantile of `members` sorted values lies -- between values lo and lo + 1, the fraction
    frac of the way; numpy's default linear position (fluid_quantile_position: host logic, no device)."""
    lo, frac = C.c_int(), C.c_double()
    capi.check(capi.lib().fluid_quantile_position(int(members), float(level), C.byref(lo), C.byref(frac)))
    return lo.value, frac.value


def coefficients(n, dt, coef):
    a, b = C.c_float(), C.c_float()
    capi.check(capi.lib().fluid_coefficients(n, dt, coef, C.byref(a), C.byref(b)))
    return a.value, b.value


def step(N, dt, diff, visc, u, v, dens):
    """The drop-in: one loop body of the reference's main for z > 0, in place
    on host arrays (C ABI `step`, include/fluid_amd.h)."""
    for a in (u, v, dens):
        if a.dtype != np.float32 or not a.flags.c_contiguous or a.shape != (N + 2, N + 2):
            raise ValueError("fields must be C-contiguous float32 of shape (N+2, N+2)")
    capi.check(capi.lib().step(N, dt, diff, visc, u, v, dens))


def step_src(N, dt, diff, visc, iters, u, v, dens, u_prev, v_prev, dens_prev):
    for a in (u, v, dens, u_prev, v_prev, dens_prev):
        if a.dtype != np.float32 or not a.flags.c_contiguous or a.shape != (N + 2, N + 2):
            raise ValueError("fields must be C-contiguous float32 of shape (N+2, N+2)")
    capi.check(capi.lib().step_src(N, dt, diff, visc, iters, u, v, dens, u_prev, v_prev, dens_prev))
