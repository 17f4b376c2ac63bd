"""TEST HELPER: the expectation of the tide (include/pomgpu.h "tides"), independent of the library.

Forcing: the CPU oracle driven routine by routine; before each of its mode_external calls the state's eight boundary lines are base + tide,
afterwards base again.  The tide is formed here with math.cos / math.sin (the C library's) in the header's order:
e = e + (elC * cw + elS * sw), constituent after constituent.  Analysis: a numpy restatement of the sums and of the normal matrix."""
import math

import numpy as np

from oracle.pyoracle import OracleTile

SIDES = ("east", "south", "west", "north")
EL = {"east": "ele", "south": "els", "west": "elw", "north": "eln"}
UN = {"east": "uabe", "south": "vabs", "west": "uabw", "north": "vabn"}
# M2 S2 N2 K2 K1 O1 P1 Q1, rad/s
OMEGA = (1.405189e-4, 1.454441e-4, 1.378797e-4, 1.458423e-4, 0.729212e-4, 0.675977e-4, 0.725229e-4, 0.649585e-4)


def tide_time(st, iint, iext):
    return (float(st.time0) * 86400.0 + float(st.dti) * float(iint - 1)) + float(st.dte) * float(iext)


def phasors(omega, t):
    """[(cos(omega t), sin(omega t))] with the C library's functions"""
    return [(math.cos(w * t), math.sin(w * t)) for w in omega]


def make_lines(nc, im_global, jm_global, with_un=True, sides=SIDES, seed=0, scale=1.0):
    """per side dict(el_amp, el_pha[, un_amp, un_pha]), (nc, n_global) each: smooth along the line, different per side and constituent,
    a function of the GLOBAL index alone"""
    out = {}
    for s, name in enumerate(SIDES):
        if name not in sides:
            continue
        n = jm_global if name in ("east", "west") else im_global
        a = np.arange(1, n + 1, dtype=np.float64)[None, :]
        c = np.arange(1, nc + 1, dtype=np.float64)[:, None]
        d = dict(el_amp=scale * (0.05 + 0.02 * np.sin(0.37 * a + c + s + seed)) / c, el_pha=np.mod(40.0 * c + 3.0 * a + 70.0 * s + 11.0 * seed, 360.0))
        if with_un:
            d.update(un_amp=scale * (0.004 + 0.002 * np.cos(0.23 * a + 2.0 * c + s)) / c, un_pha=np.mod(25.0 * c + 2.0 * a + 50.0 * s + 7.0 * seed, 360.0))
        out[name] = d
    return out


def coefficients(lines, nc, im_global, jm_global):
    """{side: (elC, elS, unC, unS)}, (nc, n_global) each: C = A cos g, S = A sin g with g in degrees, restated here (not the host
    layer's function: a wrong sign there must show); no un lines: zeros"""
    def cs(amp, pha):
        amp, g = np.asarray(amp, dtype=np.float64), np.asarray(pha, dtype=np.float64) * (math.pi / 180.0)
        return amp * np.vectorize(math.cos)(g), amp * np.vectorize(math.sin)(g)
    out = {}
    for name, d in lines.items():
        n = jm_global if name in ("east", "west") else im_global
        elC, elS = cs(d["el_amp"], d["el_pha"])
        unC, unS = cs(d["un_amp"], d["un_pha"]) if "un_amp" in d else (np.zeros((nc, n)), np.zeros((nc, n)))
        out[name] = tuple(np.ascontiguousarray(x, dtype=np.float64) for x in (elC, elS, unC, unS))
    return out


def add_tide(st, coef, ph):
    """base + tide in the eight lines of the state; returns what to put back"""
    base = {}
    for name, (elC, elS, unC, unS) in coef.items():
        alongj = name in ("east", "west")
        n, g0 = (st.jm, st.j_off) if alongj else (st.im, st.i_off)
        for field, (C, S) in ((EL[name], (elC, elS)), (UN[name], (unC, unS))):
            line = st.field(field)
            base[field] = line.copy()
            e = line[:n].copy()
            for c, (cw, sw) in enumerate(ph):
                e = e + (C[c, g0:g0 + n] * cw + S[c, g0:g0 + n] * sw)
            line[:n] = e
    return base


def restore(st, base):
    for field, x in base.items():
        st.field(field)[...] = x


def oracle_steps(st, omega, coef, nsteps):
    """nsteps internal steps of the oracle with the tide in bcond(2), routine by routine (advance.f:6-59)"""
    ot = OracleTile(st)
    isplit = int(st.isplit)
    for _ in range(nsteps):
        st.iint = int(st.iint) + 1
        ot.call("get_time")
        ot.call("lateral_viscosity")
        ot.call("mode_interaction")
        for iext in range(1, isplit + 1):
            st.iext = iext
            base = add_tide(st, coef, phasors(omega, tide_time(st, int(st.iint), iext)))
            ot.call("mode_external")
            restore(st, base)
        st.iext = isplit + 1
        ot.call("mode_internal")
        ot.call("check_velocity")
    return st


# ---- the analysis --------------------------------------------------------------------------------------------------------------------------
def sample_time(st, iint):
    return float(st.time0) * 86400.0 + float(st.dti) * float(iint)


def basis(omega, t):
    b = [1.0]
    for cw, sw in phasors(omega, t):
        b += [cw, sw]
    return np.array(b)


def accumulate_field(sums, f, b):
    """what k_harm_accum adds for one sample of one field: sums[0] = sums[0] + f, sums[p] = sums[p] + f * b[p]"""
    sums[0] = sums[0] + f
    for p in range(1, b.size):
        sums[p] = sums[p] + f * b[p]


def accumulate_matrix(M, b):
    """what the host adds for one sample: M = M + b b^T, row by row"""
    for p in range(b.size):
        for q in range(b.size):
            M[p, q] = M[p, q] + b[p] * b[q]
