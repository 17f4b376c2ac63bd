"""TEST HELPER: the tracers' files, means and inventory (include/pomgpu.h: pomgpu_write_tracers, pomgpu_read_tracers, pomgpu_tracer_stats,
pomgpu_tracer_mean_*; no counterpart in the reference).

Shared by tests/test_tracer_files_emulated.py (host build of the kernel sources) and tests/test_gpu_tracer_files.py (the device): every
check takes the library to load (None: the product library on device 0).  What a tracer does in a step is held to tests/tracer_expect.py
by tests/tracer_checks.py; this suite pins what is written, what is read back, what is accumulated and what is summed.  Files are read
with scipy.io.netcdf_file, hand-made inputs are written with it (version=2: CDF-2).  Comparisons of arrays are on 64-bit patterns; the
two sums of the inventory are held to rtol 1e-12, the bar test_domain_stats_on_device sets for the same reduction tree: with all-positive
inputs the tree's own error is about (kbm1 + log2(threads)) * 2^-53, some 4e-15, so the bar can only hide a wrong term."""
import json
import math
import os

import numpy as np

import mean_output_checks as moc
from tracer_checks import ARRAYS, independent, put
from uv_tail_fused_checks import diff, same_bits, start
from extpom_amd.model import PomGpu
from extpom_amd.lib import PomGpuError

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [(9, 8, 5), (11, 7, 5), (20, 17, 6), (65, 49, 21)]    # n3 even; n2 and n3 odd (a tail element); the tracer suites' middle size; odd a3
KW = dict(title="tracers", time_start="2000-01-01 00:00:00 +00:00")
ADDED_LAUNCHES_PER_STEP = 1                                   # include/pomgpu.h: k_mean_accum once more per step, with the tracers' table


def nn(stem, n):
    return "%s%02d" % (stem, n)


def read_file(path):
    from scipy.io import netcdf_file
    with netcdf_file(str(path), "r", mmap=False) as f:
        return {k: np.array(v.data, dtype=np.float64) for k, v in f.variables.items()}


def refused(fn, *words):
    try:
        fn()
    except PomGpuError as e:
        assert all(w in str(e) for w in words), str(e)
        return
    raise AssertionError("not refused: " + " / ".join(words))


def context(lib, case, size, ntr, adv=(2, 1), warm=2, seed=7, tracers=True):
    """a started state with ntr independent tracers registered: (state, context, tracers)"""
    _, b = start(case, dict(nadv=adv[0], nitera=adv[1]), size, warm=warm)
    g = PomGpu(b, libpath=lib)
    trs = [independent(b, seed=seed + n, nbc=1 if n % 2 == 0 else 3, source=n != 1, clim=n != 2) for n in range(ntr)]
    if tracers:
        g.set_tracers(ntr)
        for n, t in enumerate(trs, 1):
            put(g, n, t)
    return b, g, trs


def patch(st, x):
    return x[..., :st.jm, :st.im]


# ---- the header against tests/golden/tracer_file_schema.json ---------------------------------------------------------------------------
def check_header(path, kind, ntr, st, title=KW["title"], time_start=KW["time_start"], im_global=None, jm_global=None):
    from scipy.io import netcdf_file
    schema = json.load(open(os.path.join(HERE, "golden", "tracer_file_schema.json")))
    want = schema[kind]
    sizes = {"kb": st.kb, "kbm1": st.kb - 1, "im_global": im_global or st.im, "jm_global": jm_global or st.jm}
    fill = lambda t, n: t.replace("{title}", title).replace("{time_start}", time_start).replace("{NN}", "%02d" % n)
    vars_ = []
    for sec in want["sections"]:
        for n in (range(1, ntr + 1) if sec["per_tracer"] else [0]):
            vars_ += [(fill(v["name"], n), v["dims"], [[k, fill(t, n)] for k, t in v["atts"]]) for v in sec["vars"]]
    with netcdf_file(str(path), "r", mmap=False) as f:
        assert f.version_byte == schema["version_byte"], f.version_byte
        got_g = [[k, v.decode() if isinstance(v, bytes) else v] for k, v in f._attributes.items()]
        assert got_g == [[k, fill(v, 0)] for k, v in want["global_atts"]], got_g
        assert [[k, v] for k, v in f.dimensions.items()] == [[k, v if isinstance(v, int) else sizes[v]] for k, v in want["dims"]], f.dimensions
        assert list(f.variables) == [v[0] for v in vars_], list(f.variables)
        for name, dims, atts in vars_:
            g = f.variables[name]
            assert list(g.dimensions) == dims, (name, g.dimensions)
            assert g.typecode() == "d" and g.data.dtype.str == ">f8", (name, g.typecode())
            got_a = [[k, a.decode() if isinstance(a, bytes) else a] for k, a in g._attributes.items()]
            assert got_a == atts, (name, got_a)


# ---- hand-made input files ----------------------------------------------------------------------------------------------------------------
def hand_file(path, st, arrays, scalars=None, dtype="d", kb=None, record=False):
    """a CDF-2 file an outside tool would write: arrays {name: (kb, jm, im) values} as (z, y, x) variables -- `record`: behind an unlimited
    dimension; dtype "f": NC_FLOAT -- and scalars {name: value}"""
    from scipy.io import netcdf_file
    kb = kb or st.kb
    jm, im = st.jm, st.im
    with netcdf_file(str(path), "w", version=2) as f:
        if record:
            f.createDimension("time", None)
        f.createDimension("z", kb)
        f.createDimension("y", jm)
        f.createDimension("x", im)
        for name, x in (scalars or {}).items():
            v = f.createVariable(name, "d", ())
            v[...] = float(x)
        for name, x in arrays.items():
            v = f.createVariable(name, dtype, (("time",) if record else ()) + ("z", "y", "x"))
            if record:
                v[0] = x
            else:
                v[:] = x
    return path


def random_tracer(st, rng, scale=1.0):
    """(kb, jm_local, im_local) values whose eight bytes all differ from cell to cell, level kb included, with a -0.0"""
    x = scale * rng.standard_normal((st.kb, st.jm_local, st.im_local)) * 10.0 ** rng.integers(-3, 4, (st.kb, st.jm_local, st.im_local))
    x[0, 1, 1] = -0.0
    x[st.kb - 1, 2, 2] = -0.0
    return x


def tracer_state(g, ntr, with_config=True):
    out = {}
    for n in range(1, ntr + 1):
        for name in (ARRAYS if with_config else ("trb", "tr")):
            out[(n, name)] = g.tracer_download(n, name)
        if with_config:
            out[(n, "source")] = g.tracer_download(n, "source")
            out[(n, "set")] = np.array(g.tracer_get(n), dtype=np.float64)
    return out


def same_state(x, y):
    return [k for k in x if not same_bits(x[k], y[k])]


# ---- 1: round trip, every element ---------------------------------------------------------------------------------------------------------
def round_trip(lib, tmp, size, ntr, case="archipelago"):
    b, g, _ = context(lib, case, size, ntr, adv=(2, 2))
    g.run(2)                                                  # the work array trf holds what the steps left
    rng = np.random.default_rng(int(np.prod(size)) + ntr)
    for n in range(1, ntr + 1):
        g.tracer_upload(n, "trb", random_tracer(b, rng))
        g.tracer_upload(n, "tr", random_tracer(b, rng))
        g.set_tracer(n, nbc=3 if n % 2 else 1, decay=1.0e-5 * n + 1.0e-9)
    g.get_con()
    want = tracer_state(g, ntr)
    p1, p2 = tmp / "a.tracer.rst.nc", tmp / "b.tracer.rst.nc"
    g.write_file("tracer_restart", p1, **KW)
    g.io_wait()
    check_header(p1, "restart", ntr, b)
    v = read_file(p1)
    assert v["iint"] == float(b.iint) and v["time"][0] == float(b.time) and v["ntr"] == float(ntr), (v["iint"], v["time"], v["ntr"])
    kb, jm, im = b.kb, b.jm, b.im
    for n in range(1, ntr + 1):
        assert v[nn("nbc", n)] == want[(n, "set")][0] and same_bits(np.atleast_1d(v[nn("lam", n)]), want[(n, "set")][1:2]), n
        for arr in ("tr", "trb"):
            assert v[nn(arr, n)].shape == (kb, jm, im)
            assert same_bits(v[nn(arr, n)], patch(b, want[(n, arr)])), (n, arr)
        assert np.any(v[nn("trf", n)][:kb - 1] != 0.) and not np.any(v[nn("trf", n)][kb - 1] != 0.), n   # the work array as the steps left it
        assert np.any(v[nn("tr", n)][kb - 1] != 0.)
    # a fresh context: the same bits in every array the file carries, trf shown by the file it writes in turn
    c = b.copy()
    h = PomGpu(c, libpath=lib)
    h.set_tracers(ntr)
    time_iint = h.read_tracers(p1)
    assert time_iint == (float(b.time), float(b.iint)), time_iint
    got = tracer_state(h, ntr)
    for n in range(1, ntr + 1):
        for arr in ("tr", "trb"):
            assert same_bits(patch(b, got[(n, arr)]), patch(b, want[(n, arr)])), (n, arr)
        assert same_bits(got[(n, "set")], want[(n, "set")]), (n, got[(n, "set")])
    h.write_file("tracer_restart", p2, **KW)
    h.io_wait()
    assert open(p1, "rb").read() == open(p2, "rb").read()
    h.close()
    g.close()


def initial_file(lib, tmp, size=(20, 17, 6), case="archipelago"):
    """a file with tr01 alone: trb = tr in bits, and trf = tr -- one more step at nitera = 2 equals the step of a context that read a file
    with the three arrays spelled out"""
    x = 1.0 + 0.5 * np.random.default_rng(5).random((size[2], size[1], size[0]))
    x[0, 3, 3] = -0.0
    out = []
    for full in (False, True):
        b, g, _ = context(lib, case, size, 1, adv=(2, 2))
        names = ("tr01", "trb01", "trf01") if full else ("tr01",)
        p = hand_file(tmp / ("init_%d.nc" % full), b, {k: x for k in names})
        assert g.read_tracers(p) == (0.0, 0.0)                # no time, no iint in the file
        assert same_bits(patch(b, g.tracer_download(1, "tr")), x) and same_bits(patch(b, g.tracer_download(1, "trb")), x)
        assert g.tracer_get(1) == (1, 2.0e-5)                 # nbc, lam absent: as they were (tracer_checks.independent)
        g.run(1)
        out.append(tracer_state(g, 1, with_config=False))
        g.close()
    assert not same_state(out[0], out[1]), same_state(out[0], out[1])
    assert np.isfinite(out[0][(1, "tr")]).all()


# ---- 2: the file is the state ----------------------------------------------------------------------------------------------------------------
def file_is_the_state(lib, tmp, case, size, adv, ntr=2):
    kbm1 = size[2] - 1
    a, ga, ta = context(lib, case, size, ntr, adv)
    b, gb, tb = context(lib, case, size, ntr, adv)
    ga.run(3)
    gb.run(3)
    p = tmp / "state.tracer.rst.nc"
    ga.write_file("tracer_restart", p, **KW)
    ga.io_wait()
    gb.set_tracers(ntr)                                       # everything of the tracers' to +0.0, trf included
    assert not np.any(gb.tracer_download(1, "tr"))
    for n, t in enumerate(tb, 1):
        put(gb, n, t)                                         # the configuration arrays (and the START's trb, tr, which the file replaces)
    assert not same_bits(gb.tracer_download(1, "tr")[:kbm1], ga.tracer_download(1, "tr")[:kbm1])
    gb.read_tracers(p)
    ga.run(3)
    gb.run(3)
    for n in range(1, ntr + 1):
        for arr in ("tr", "trb"):
            x, y = ga.tracer_download(n, arr)[:kbm1], gb.tracer_download(n, arr)[:kbm1]
            assert same_bits(x, y), (adv, n, arr, int(np.count_nonzero(x != y)))
            assert np.isfinite(x).all()
    ga.download()
    gb.download()
    assert not diff(a, b), diff(a, b)                         # tracers never write the flow
    ga.close()
    gb.close()


# ---- 3: the output kind -------------------------------------------------------------------------------------------------------------------
def output_kind(lib, tmp, size=(20, 17, 6), ntr=3, case="archipelago"):
    b, g, _ = context(lib, case, size, ntr)
    g.run(3)
    kbm1 = b.kb - 1
    stats = g.tracer_stats()
    snap, own, given = tmp / "flow.nc", tmp / "own.tracer.nc", tmp / "given.tracer.nc"
    g.write_file("output", snap, **KW)
    g.io_wait()
    g.write_file("tracer_output", own, **KW)
    g.io_wait()
    handed = np.arange(1.0, 4 * ntr + 1).reshape(ntr, 4) / 7.0
    g.write_file("tracer_output", given, trstats=handed, **KW)
    g.io_wait()
    check_header(own, "output", ntr, b)
    check_header(given, "output", ntr, b)
    flow, vo, vg = read_file(snap), read_file(own), read_file(given)
    for k in ("time", "z", "zz"):
        assert same_bits(vo[k], flow[k]) and same_bits(vg[k], flow[k]), k
    for n in range(1, ntr + 1):
        tr = patch(b, g.tracer_download(n, "tr"))[:kbm1]
        for v in (vo, vg):
            assert v[nn("tr", n)].shape == (1, kbm1, b.jm, b.im)
            assert same_bits(v[nn("tr", n)][0], tr), n
        for q, stem in enumerate(("tot", "avg", "min", "max")):
            assert same_bits(vo[nn(stem, n)], stats[n - 1, q:q + 1]), (n, stem)
            assert same_bits(vg[nn(stem, n)], handed[n - 1, q:q + 1]), (n, stem)
    assert np.any(vo["tr01"] != 0.)
    g.close()


# ---- 4: means -------------------------------------------------------------------------------------------------------------------------------
class Twin:
    """acc = acc + tr per step from +0.0 for every tracer, tr downloaded from a twin context that runs one step at a time"""

    def __init__(self, lib, case, size, ntr, adv=(2, 1)):
        self.st, self.g, _ = context(lib, case, size, ntr, adv)
        self.ntr = ntr
        self.reset()

    def reset(self):
        self.acc = [np.zeros(self.g.tracer_shape("tr")) for _ in range(self.ntr)]
        self.n = 0

    def step(self, count=1, accumulate=True):
        for _ in range(count):
            self.g.run(1)
            if accumulate:
                for n in range(self.ntr):
                    self.acc[n] = self.acc[n] + self.g.tracer_download(n + 1, "tr")
                self.n += 1

    def mean(self, n):
        return self.acc[n - 1] / float(self.n)


def wrong_means(g, want):
    return [n for n in range(1, want.ntr + 1) if not same_bits(patch(g.st, g.tracer_mean(n)), patch(g.st, want.mean(n)))]


def mean_file(lib, tmp, chained, case="archipelago", size=(20, 17, 6), ntr=3):
    want = Twin(lib, case, size, ntr)
    b, g, _ = context(lib, case, size, ntr)
    kbm1 = b.kb - 1
    g.set_mean_output(True)
    assert g.tracer_mean_count() == 0 and g.mean_count() == 0
    g.run(7)
    want.step(7)
    for cnt, tag in ((7, "a"), (3, "b")):
        assert g.tracer_mean_count() == cnt and g.mean_count() == 7 + (3 if tag == "b" else 0)
        assert not wrong_means(g, want), wrong_means(g, want)
        means = [g.tracer_mean(n) for n in range(1, ntr + 1)]
        assert g.tracer_mean_count() == cnt                   # reading a mean resets nothing
        snap, mean = tmp / f"snap_{tag}.tracer.nc", tmp / f"mean_{tag}.tracer.nc"
        g.write_file("tracer_output", snap, **KW)
        assert g.tracer_mean_count() == cnt                   # the snapshot file leaves the sums alone
        g.write_file("tracer_output_mean", mean, **KW)
        assert g.tracer_mean_count() == 0 and g.mean_count() == 7 + (3 if tag == "b" else 0)   # the nine fields' count is their file's
        if tag == "a":
            if not chained:
                g.io_wait()
            g.run(3)                                          # chained: enqueued while the writer's thread still copies the snapshot
            want.reset()
            want.step(3)
        g.io_wait()
        check_header(mean, "output", ntr, b)
        vs, vm = read_file(snap), read_file(mean)
        assert list(vs) == list(vm)
        for k in vs:
            if k.startswith("tr"):
                n = int(k[2:])
                assert same_bits(vm[k][0], patch(b, means[n - 1])[:kbm1]), (tag, k)
                assert not same_bits(vm[k], vs[k]), (tag, k)
            else:
                assert same_bits(vs[k], vm[k]), (tag, k)
    g.close()
    want.g.close()


def nine_fields_unchanged(lib, tmp, case="archipelago", size=(20, 17, 6)):
    """mean(name) of the nine fields and the output_mean file, with and without tracers registered"""
    out = []
    for tracers in (False, True):
        b, g, _ = context(lib, case, size, 3, tracers=tracers)
        g.set_mean_output(True)
        g.run(5)
        means = {k: g.mean(k) for k in PomGpu.MEAN_FIELDS}
        p = tmp / ("nine_%d.nc" % tracers)
        g.write_file("output_mean", p, **KW)
        g.io_wait()
        assert g.mean_count() == 0 and g.tracer_mean_count() == (5 if tracers else -1)   # the nine fields' file leaves the tracers' sums alone
        out.append((means, open(p, "rb").read()))
        g.close()
    assert not [k for k in PomGpu.MEAN_FIELDS if not same_bits(out[0][0][k], out[1][0][k])]
    assert out[0][1] == out[1][1] and len(out[0][1]) > 1000


def allocation_rules(lib, case="archipelago", size=(20, 17, 6)):
    want = Twin(lib, case, size, 2)
    b, g, trs = context(lib, case, size, 2, tracers=False)
    assert g.tracer_mean_count() == -1
    g.set_mean_output(True)
    assert g.tracer_mean_count() == -1 and g.mean_count() == 0     # the mean on, no tracers: no tracer accumulators
    refused(lambda: g.tracer_mean(1), "no tracers")
    g.set_tracers(2)
    for n, t in enumerate(trs, 1):
        put(g, n, t)
    assert g.tracer_mean_count() == 0
    g.run(2)
    want.step(2)
    assert g.tracer_mean_count() == 2 and g.mean_count() == 2 and not wrong_means(g, want)
    nine = {k: g.mean(k) for k in PomGpu.MEAN_FIELDS}
    # set_tracers while the mean is on: the tracers' sums and count from zero, the nine fields' untouched
    g.set_tracers(2)
    assert g.tracer_mean_count() == 0 and g.mean_count() == 2
    assert not [k for k in PomGpu.MEAN_FIELDS if not same_bits(nine[k], g.mean(k))]
    for n in (1, 2):
        put(g, n, dict(trs[n - 1], tr=want.g.tracer_download(n, "tr"), trb=want.g.tracer_download(n, "trb")))
    # (the twin's work array differs from this context's zeroed one: nitera = 1 does not read it across steps)
    g.run(1)
    want.reset()
    want.step(1)
    assert g.tracer_mean_count() == 1 and g.mean_count() == 3 and not wrong_means(g, want)
    g.set_mean_output(True)                                   # twice: both from zero
    assert g.tracer_mean_count() == 0 and g.mean_count() == 0
    g.set_mean_output(True)
    want.reset()
    assert g.tracer_mean_count() == 0 and g.mean_count() == 0
    g.run(3)
    want.step(3)
    assert g.tracer_mean_count() == 3 and not wrong_means(g, want)
    g.set_tracers(0)
    assert g.tracer_mean_count() == -1 and g.mean_count() == 3
    g.set_tracers(1)
    assert g.tracer_mean_count() == 0
    g.set_mean_output(False)
    assert g.tracer_mean_count() == -1 and g.mean_count() == -1 and g.tracer_count() == 1
    refused(lambda: g.tracer_mean(1), "off")
    g.run(1)
    g.close()
    want.g.close()


def every_element(lib, size, ntr=3):
    """the accumulation alone: three accumulations of uploaded random tr through the entry point, no step in between -- EVERY element of
    every accumulator, level kb and the padding included"""
    b, g, _ = context(lib, "seamount", size, ntr)
    g.set_mean_output(True)
    rng = np.random.default_rng(int(np.prod(size)))
    acc = [np.zeros(g.tracer_shape("tr")) for _ in range(ntr)]
    for _ in range(3):
        for n in range(ntr):
            x = random_tracer(b, rng)
            g.tracer_upload(n + 1, "tr", x)
            acc[n] = acc[n] + x
        g.mean_accumulate()
    assert g.tracer_mean_count() == 3 and g.mean_count() == 3
    bad = [n for n in range(ntr) if not same_bits(g.tracer_mean(n + 1), acc[n] / 3.)]
    assert not bad, bad
    g.close()


# ---- 5: the inventory -------------------------------------------------------------------------------------------------------------------------
def restated_stats(st, trb, tr):
    """tot (math.fsum over the formula's cells), avg = tot / vtot, min, max"""
    kbm1, im, jm = st.kb - 1, st.im, st.jm
    dvol = (st.dx * st.dy * st.fsm * st.dt)[None, :, :] * st.dz[:kbm1, None, None]
    inner = (slice(0, kbm1), slice(1, jm - 1), slice(1, im - 1))
    tot = math.fsum((trb[:kbm1] * dvol)[inner].ravel())
    vtot = math.fsum(dvol[inner].ravel())
    wet = np.broadcast_to(st.fsm[None, :jm, :im] != 0., (kbm1, jm, im))
    x = tr[:kbm1, :jm, :im][wet]
    return tot, tot / vtot, float(x.min()), float(x.max())


def inventory(lib, size, ntr, case="archipelago", land_huge=False):
    b, g, _ = context(lib, case, size, ntr)
    g.run(2)
    g.download()
    rng = np.random.default_rng(int(np.prod(size)) + 100 * ntr)
    fields = []
    for n in range(1, ntr + 1):
        trb, tr = 1.0 + 0.5 * rng.random(g.tracer_shape("tr")), 1.0 + 0.5 * rng.random(g.tracer_shape("tr"))
        if land_huge:
            land = np.broadcast_to(b.fsm[None] == 0., trb.shape)
            assert land.any()
            trb[land], tr[land] = 1.0e300, -1.0e300
        g.tracer_upload(n, "trb", trb)
        g.tracer_upload(n, "tr", tr)
        fields.append((trb, tr))
    got, again = g.tracer_stats(), g.tracer_stats()
    assert same_bits(got, again)                              # same launch, same bits
    for n, (trb, tr) in enumerate(fields):
        tot, avg, mn, mx = restated_stats(b, trb, tr)
        print(f"inventory {size} tracer {n + 1}: tot rel {abs(got[n, 0] - tot) / abs(tot):.3e} avg rel {abs(got[n, 1] - avg) / abs(avg):.3e}")
        assert abs(got[n, 0] - tot) <= 1.0e-12 * abs(tot), (n, got[n, 0], tot)
        assert abs(got[n, 1] - avg) <= 1.0e-12 * abs(avg), (n, got[n, 1], avg)
        assert got[n, 2] == mn and got[n, 3] == mx, (n, got[n, 2:], mn, mx)
        assert 1.0 <= avg <= 1.5 and tot > 0.
    g.close()


def decay_does_not_grow(lib, size=(20, 17, 6)):
    """a sanity check, not a bar: a decaying tracer with no source in a closed basin does not gain inventory in 4 steps"""
    _, b = start("basin", None, size, warm=2)
    g = PomGpu(b, libpath=lib)
    g.set_tracers(1)
    x = np.ones(g.tracer_shape("tr"))
    g.tracer_upload(1, "trb", x)
    g.tracer_upload(1, "tr", x)
    g.set_tracer(1, nbc=1, decay=1.0e-4)
    before = g.tracer_stats()[0, 0]
    g.run(4)
    after = g.tracer_stats()[0, 0]
    assert 0. < after <= before, (before, after)
    g.close()


# ---- 6: refusals ----------------------------------------------------------------------------------------------------------------------------
def refusals(lib, tmp, size=(9, 8, 5)):
    b, g, _ = context(lib, "seamount", size, 2, tracers=False)
    x = 1.0 + np.arange(b.kb * b.jm * b.im, dtype=np.float64).reshape(b.kb, b.jm, b.im) / 7.0
    good = hand_file(tmp / "good.nc", b, {"tr01": x, "tr02": 2.0 * x})
    refused(lambda: g.read_tracers(good), "no tracers are registered")
    refused(lambda: g.write_file("tracer_restart", tmp / "none.nc"), "no tracers are registered")
    refused(lambda: g.tracer_stats(), "no tracers are registered")
    assert not os.path.exists(tmp / "none.nc")
    g.set_con(error_status=0)
    g.set_tracers(2)
    trs = [independent(b, seed=61 + n, nbc=1 if n == 0 else 3) for n in range(2)]
    for n, t in enumerate(trs, 1):
        put(g, n, t)
    g.set_mean_output(True)
    g.run(2)
    before_flow = g.download().copy()
    before = tracer_state(g, 2)
    means = [g.tracer_mean(n) for n in (1, 2)]

    def unchanged(tcount=2, count=2):
        assert g.tracer_mean_count() == tcount and g.mean_count() == count
        assert not same_state(before, tracer_state(g, 2)), same_state(before, tracer_state(g, 2))
        now = b.copy()
        g.download(now)
        assert not moc.diff(before_flow, now), moc.diff(before_flow, now)
        if tcount > 0:
            assert all(same_bits(means[n - 1], g.tracer_mean(n)) for n in (1, 2))
        assert int(now.error_status) == 1                     # every refusal raises the reference's error flag
        g.set_con(error_status=0)

    def bytes_patched(src, dst, at, new):
        raw = bytearray(open(src, "rb").read())
        raw[at:at + len(new)] = new
        open(dst, "wb").write(bytes(raw))
        return dst

    cases = [
        (hand_file(tmp / "one.nc", b, {"tr01": x}), ("variable tr02 is absent",)),
        (hand_file(tmp / "float.nc", b, {"tr01": x, "tr02": x}, dtype="f"), ("tr01", "NetCDF type 5", "NC_DOUBLE")),
        (hand_file(tmp / "levels.nc", b, {"tr01": np.ones((b.kb + 1, b.jm, b.im)), "tr02": np.ones((b.kb + 1, b.jm, b.im))}, kb=b.kb + 1), ("tr01", "dimension lengths")),
        (hand_file(tmp / "record.nc", b, {"tr01": x, "tr02": x}, record=True), ("tr01", "record variable")),
        (bytes_patched(good, tmp / "cdf5.nc", 3, b"\x05"), ("CDF version 5",)),
        (hand_file(tmp / "nbc.nc", b, {"tr01": x, "tr02": x}, scalars={"nbc01": 2.0}), ("nbc01", "1 (the flux")),
    ]
    for path, words in cases:
        refused(lambda: g.read_tracers(path), *words)
        unchanged()
    raw = open(good, "rb").read()
    open(tmp / "short.nc", "wb").write(raw[:len(raw) - 8])
    refused(lambda: g.read_tracers(tmp / "short.nc"), "reaches beyond the file")
    unchanged()
    open(tmp / "hdf5.nc", "wb").write(b"\x89HDF\r\n\x1a\n" + raw[8:])
    refused(lambda: g.read_tracers(tmp / "hdf5.nc"), "HDF5")
    unchanged()
    refused(lambda: g.read_tracers(good, im_global=b.im - 1), "does not fit the global grid")
    unchanged()
    refused(lambda: g.write_file("tracer_output", tmp / "misfit.nc", im_global=b.im - 1), "does not fit the global grid")
    unchanged()
    bad_kind = lambda: g._chk(g.L.pomgpu_write_tracers(g.h, str(tmp / "kind.nc").encode(), _meta(b), 3, None), "write_tracers")
    refused(bad_kind, "kind = 3")
    unchanged()
    # the mean kind with count 0, and with the mean off: no file is touched
    g.set_mean_output(True)
    before_flow = g.download().copy()
    refused(lambda: g.write_file("tracer_output_mean", tmp / "zero.nc"), "no step")
    unchanged(0, 0)
    g.set_mean_output(False)
    refused(lambda: g.write_file("tracer_output_mean", tmp / "off.nc"), "mean output is off")
    unchanged(-1, -1)
    assert not any(os.path.exists(tmp / n) for n in ("misfit.nc", "kind.nc", "zero.nc", "off.nc"))
    # and the accepted file is still accepted
    g.read_tracers(good)
    assert same_bits(patch(b, g.tracer_download(2, "trb")), 2.0 * x)
    g.run(1)
    g.close()


def _meta(st):
    import ctypes
    from extpom_amd import lib as _lib
    return ctypes.byref(_lib.FileMeta(b"", b"", st.im, st.jm, st.i_off + 1, st.j_off + 1, 1, None))


def fp32_builds_refuse(lib_f32, tmp, size=(9, 8, 5)):
    _, b = start("seamount", None, size)
    g = PomGpu(b, libpath=lib_f32)
    x = np.ones((b.kb, b.jm, b.im))
    p = hand_file(tmp / "f32.nc", b, {"tr01": x})
    refused(lambda: g.read_tracers(p), "fp32-storage variant")
    refused(lambda: g.write_file("tracer_restart", tmp / "f32_out.nc"), "fp32-storage variant")
    refused(lambda: g._chk(g.L.pomgpu_tracer_stats(g.h, None), "tracer_stats"), "fp32-storage variant")
    refused(lambda: g.tracer_get(1), "fp32-storage variant")
    assert g.tracer_mean_count() == -1 and not os.path.exists(tmp / "f32_out.nc")
    g.close()


# ---- 8: tiles -------------------------------------------------------------------------------------------------------------------------------
def tiles(lib, nx, ny, tmp, case="archipelago", ntr=2, more=2):
    """nx x ny tiles (tests/tracer_checks.py: run_tiles' set-up) write ONE restart-kind and ONE output-kind file, the rank with create = 1
    first; both equal the single tile's files on every cell.  Each rank then zeroes its tracers, reads its patch back -- ghost lines
    included, no message round -- and continues `more` steps: equal to the single tile on owned cells.  No new call adds a message round;
    the tiles' tot add up to the single tile's"""
    import threading
    import tracer_checks as tc
    from extpom_amd import decomp
    from extpom_amd.cases import finish_initial, make_case
    from forcing_files_checks import Board, device_mover, host_mover
    from oracle.pyoracle import oracle_finish_initial
    mover = host_mover if lib is not None else device_mover
    IMg, JMg = tc.TILE_GRID
    kb, kbm1 = tc.TILE_KB, tc.TILE_KB - 1
    glob = dict(im_global=IMg, jm_global=JMg)
    one = make_case(case, IMg, JMg, kb, dte=6.0, isplit=tc.TILE_ISPLIT)
    oracle_finish_initial(one)
    g = PomGpu(one, libpath=lib)
    g.set_tracers(ntr)
    for n in range(1, ntr + 1):
        put(g, n, independent(one, seed=50 + n, nbc=1 if n != 2 else 3))
    g.run(tc.TILE_STEPS)
    stats1 = g.tracer_stats()
    g.write_file("tracer_restart", tmp / "one.rst.nc", **KW)
    g.io_wait()
    g.write_file("tracer_output", tmp / "one.out.nc", trstats=stats1, **KW)
    g.io_wait()
    g.run(more)
    single = {(n, k): g.tracer_download(n, k) for n in range(1, ntr + 1) for k in ("tr", "trb")}
    g.close()

    world = nx * ny
    iml, jml = decomp.local_size(IMg, JMg, nx, ny)
    tls = [decomp.make_tile(r, IMg, JMg, iml, jml, n_proc=world) for r in range(world)]
    board, out, errs = Board(world), {}, []
    rst, outp = tmp / "tiles.rst.nc", tmp / "tiles.out.nc"

    def rank(r):
        try:
            tile = tls[r]
            st = make_case(case, IMg, JMg, kb, tile=tile, dte=6.0, isplit=tc.TILE_ISPLIT)
            stream = None
            if lib is None:
                import torch
                torch.cuda.set_device(0)
                ts = torch.cuda.Stream()
                torch.cuda.set_stream(ts)
                stream = ts.cuda_stream
            g = PomGpu(st, device=0, stream=stream, libpath=lib)
            move, ordered = mover(board, tile, g)
            g.set_transport(tile, move, agree=lambda mine: board.allmin(r, mine), stream_ordered=ordered)
            g.set_wide_external(True, min(t.im for t in tls), min(t.jm for t in tls))

            def dens(s, a, b, c):
                g.upload(s); g.call("dens", a, b, c); g.download(s)

            def baropg(s):
                g.upload(s); g.call("baropg_mcc" if int(s.npg) == 2 else "baropg"); g.download(s)

            finish_initial(st, dens, baropg)
            g.upload(st)
            board.barrier.wait()
            trs = [independent(st, seed=50 + n, nbc=1 if n != 2 else 3, i0=tile.i_off, j0=tile.j_off, gshape=(JMg, IMg)) for n in range(1, ntr + 1)]
            g.set_tracers(ntr)
            for n, t in enumerate(trs, 1):
                put(g, n, t)
            g.run(tc.TILE_STEPS)
            g.sync()
            r0 = (g.exchange_rounds(), g.exchange_rounds_side())
            stats = g.tracer_stats()
            for create in (True, False):                      # the two-pass pattern: the creating rank, a barrier, the others
                if create == (r == 0):
                    g.write_file("tracer_restart", rst, create=create, **glob, **KW)
                    g.io_wait()
                board.barrier.wait()
            for create in (True, False):
                if create == (r == 0):
                    g.write_file("tracer_output", outp, create=create, trstats=stats1, **glob, **KW)
                    g.io_wait()
                board.barrier.wait()
            g.set_tracers(ntr)
            for n, t in enumerate(trs, 1):
                put(g, n, t)
            g.read_tracers(rst, **glob)
            assert (g.exchange_rounds(), g.exchange_rounds_side()) == r0, "a new call posted a message round"
            board.barrier.wait()
            g.run(more)
            arrs = {(n, k): g.tracer_download(n, k) for n in range(1, ntr + 1) for k in ("tr", "trb")}
            g.download()
            assert int(st.error_status) == 0
            g.close()
            out[r] = (tile, arrs, stats)
        except Exception:                                     # a dead rank must not leave the others at the barrier
            import traceback
            errs.append(traceback.format_exc())
            board.barrier.abort()

    threads = [threading.Thread(target=rank, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs[0]
    for a, b in ((tmp / "one.rst.nc", rst), (tmp / "one.out.nc", outp)):
        va, vb = read_file(a), read_file(b)
        assert list(va) == list(vb)
        bad = [k for k in va if not same_bits(va[k], vb[k])]
        assert not bad, (str(b), bad)
    bad = []
    for r, (tile, arrs, stats) in out.items():
        io, jo, im, jm = tile.i_off, tile.j_off, tile.im, tile.jm
        sl_j = slice(0 if jo == 0 else 1, jm if jo + jm == JMg else jm - 1)       # the cells the tile owns
        sl_i = slice(0 if io == 0 else 1, im if io + im == IMg else im - 1)
        for key, x in arrs.items():
            ref = single[key][:kbm1, jo:jo + jm, io:io + im][:, sl_j, sl_i]
            if not same_bits(ref, x[:kbm1, :jm, :im][:, sl_j, sl_i]) or not np.isfinite(x).all():
                bad.append((r, key))
    assert not bad, bad
    for n in range(ntr):
        tot = math.fsum(out[r][2][n, 0] for r in out)
        print(f"tiles {nx}x{ny} tracer {n + 1}: summed tot rel {abs(tot - stats1[n, 0]) / abs(stats1[n, 0]):.3e}")
        assert abs(tot - stats1[n, 0]) <= 1.0e-12 * abs(stats1[n, 0]), (n, tot, stats1[n, 0])
        assert min(out[r][2][n, 2] for r in out) == stats1[n, 2] and max(out[r][2][n, 3] for r in out) == stats1[n, 3]


# ---- 7: launch counts -----------------------------------------------------------------------------------------------------------------------
def launch_counts(lib, size=(65, 49, 21), ntr=3, steps=5):
    """with the mean on and tracers registered the step launches what it launches with the mean off, k_mean_accum for the nine fields and
    ADDED_LAUNCHES_PER_STEP more for the tracers, whatever their number"""
    b, g, _ = context(lib, "seamount", size, ntr)
    g.run(2)
    g.prof_begin()
    g.run(steps)
    off = {k: n for k, (n, _) in g.prof_end().items()}
    g.set_mean_output(True)
    g.prof_begin()
    g.run(steps)
    on = {k: n for k, (n, _) in g.prof_end().items()}
    assert "k_mean_accum" not in off and on.pop("k_mean_accum") == steps * (1 + ADDED_LAUNCHES_PER_STEP), (off, on)
    assert on == off, {k: (off.get(k), on.get(k)) for k in set(on) | set(off) if off.get(k) != on.get(k)}
    assert g.tracer_mean_count() == steps
    g.prof_begin()
    g.tracer_stats()
    st = {k: n for k, (n, _) in g.prof_end().items()}
    if lib is None:                                           # (the host emulation has no lanes to shuffle between: it sums in the entry point)
        assert {k: n for k, n in st.items() if k.startswith("k_tracer")} == {"k_tracer_stats": 1, "k_tracer_stats_fin": 1}, st
    g.close()
