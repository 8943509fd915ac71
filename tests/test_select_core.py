"""CPU tier of the solver's kernel selection (csrc/obca_select.h: shape capabilities, the launch plan, "mode available"), built
for the host from tests/native/select_host.cpp.

(a) Literal pins: capability numbers and auto-mode kernels of eleven shapes, computed from the arithmetic of obca_shape_sizes,
obca_soc_lds_* and the HBM-workspace carve-up before the selection moved into the header; then the plans of the non-default
knobs.  (b) A sweep against a restatement written here from the rule as include/obca_mpc.h documents it (obca_set_mode,
obca_set_shape_specialisation, obca_set_two_sided_sweep), over the capability numbers the header reports."""
import ctypes
import itertools
import os

import numpy as np
import pytest

from tests import native_build

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "select_host.cpp")
E_LDS = -28
CAPS = ("R_max", "inst_off", "lds_bytes", "soc_lds", "lds_bytes_mw", "soc_lds_mw", "lds_bytes_gm", "gm_doubles", "inst_off_gm",
        "wave_ok", "mw_ok", "gm_ok", "n_max")
PLAN = ("rc", "kernel", "threads", "lds", "inst_off", "soc_lds", "two_sided", "needs_ws", "specialised", "available")
REFUSED = {"wave": 1, "mw": 2, "mw shape": 4, "gm": 8}

# (N, n_obs, M): R_max, inst_off, lds_bytes, soc_lds, lds_bytes_mw, soc_lds_mw, lds_bytes_gm, gm_doubles, inst_off_gm, wave / mw / gm ok, auto
PINS = {
    (5, 3, 6): (199, 3222, 30864, 3286, 32064, 3436, 9536, 6478, 978, 1, 1, 1, "wave r4"),
    (5, 5, 14): (319, 4998, 40496, 0, 49152, 5212, 9536, 12094, 978, 1, 1, 1, "wave r5"),
    (5, 6, 18): (379, 5886, 47600, 0, 57696, 6100, 9536, 12982, 978, 1, 1, 1, "wave r6"),
    (6, 6, 18): (442, 6850, 55312, 0, 66880, 7064, 10592, 13856, 1110, 0, 1, 1, "mw r3"),
    (12, 3, 6): (430, 6898, 55696, 0, 67648, 7220, 17792, 13376, 1902, 0, 1, 1, "gm1"),
    (26, 3, 6): (892, 14262, 114608, 0, 147536, 15876, 34592, 27188, 3750, 0, 1, 1, "gm1"),
    (27, 3, 6): (925, 14794, 118864, 0, 152848, 16444, 35936, 27634, 3882, 0, 1, 1, "mw r5"),
    (30, 2, 2): (714, 12150, 97712, 0, 118496, 12796, 39392, 20512, 4278, 0, 1, 1, "mw r3"),
    (20, 5, 14): (1114, 17322, 139088, 0, 161424, 0, 27392, 34616, 2958, 0, 1, 1, "mw r5"),
    (26, 5, 14): (1432, 22254, 178544, 0, 239904, 0, 34592, 42860, 3750, 0, 0, 1, "gm"),
    (127, 8, 32): (11393, 170562, 1365008, 0, 2636376, 0, 155936, 332042, 17082, 0, 0, 1, "gm"),
}


@pytest.fixture(scope="module")
def host():
    lib = native_build.build_shim("select_host", [SRC])
    lib.select_kernel_name.restype = ctypes.c_char_p
    return lib


def caps(host, N, nO, M):
    out = np.zeros(len(CAPS), np.int64)
    host.select_caps(N, nO, M, out.ctypes.data_as(ctypes.c_void_p))
    return dict(zip(CAPS, out.tolist()))


def plans(host, cases):
    """select_plans on cases [n, 11] (N, nO, M, mode, specialise, has_wave_shape, has_mw_shape, two_sided, lds_pad, gm_ws_failed,
    refused): [n, 10] in the order of PLAN"""
    cases = np.ascontiguousarray(cases, np.int64)
    out = np.zeros((len(cases), len(PLAN)), np.int64)
    host.select_plans(len(cases), cases.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
    return out


def plan(host, shape, mode=0, specialise=False, has_wave_shape=False, has_mw_shape=False, two_sided=-1, lds_pad=0, gm_ws_failed=False,
         refused=0):
    p = dict(zip(PLAN, plans(host, [list(shape) + [mode, specialise, has_wave_shape, has_mw_shape, two_sided, lds_pad, gm_ws_failed,
                                                   refused]])[0].tolist()))
    p["kernel"] = host.select_kernel_name(p["kernel"]).decode()
    return p


@pytest.mark.parametrize("shape", sorted(PINS))
def test_capabilities_and_auto_kernel_of_the_pinned_shapes(host, shape):
    want = PINS[shape]
    c = caps(host, *shape)
    assert tuple(c[k] for k in CAPS[:12]) == want[:12]
    p = plan(host, shape)
    assert p["rc"] == 0 and p["kernel"] == want[12] and not p["specialised"]


def test_row_slot_rules(host):
    assert [host.select_wave_row_slots(r) for r in (1, 256, 257, 320, 321, 384, 385)] == [4, 4, 5, 5, 6, 6, 0]
    assert [host.select_mw_row_slots(r) for r in (1, 768, 769, 1280, 1281)] == [3, 3, -5, -5, 0]


def test_instantiations_are_planned_where_the_generic_kernel_of_the_shape_would_run(host):
    on = dict(specialise=True, has_wave_shape=True, has_mw_shape=True)
    p = plan(host, (5, 3, 6), **on)
    assert (p["kernel"], p["threads"], p["lds"], p["specialised"]) == ("wave shape", 64, 30864, 1)
    p = plan(host, (20, 5, 14), **on)
    assert (p["kernel"], p["threads"], p["lds"], p["specialised"]) == ("mw shape", 256, 161424, 1)
    p = plan(host, (20, 3, 6), mode=3, **on)
    assert (p["kernel"], p["threads"], p["specialised"]) == ("mw shape", 256, 1)
    p = plan(host, (20, 3, 6), **on)
    assert (p["kernel"], p["threads"], p["specialised"], p["needs_ws"]) == ("gm1", 64, 0, 1)
    for shape in PINS:
        p = plan(host, shape, mode=2, **on)
        assert (p["rc"], p["kernel"], p["threads"], p["lds"], p["specialised"], p["needs_ws"]) == (0, "lane", 64, 0, 0, 0)
    # a refused instantiation alone is dropped: the generic four-wavefront kernel runs
    p = plan(host, (20, 5, 14), refused=REFUSED["mw shape"], **on)
    assert (p["kernel"], p["specialised"]) == ("mw r5", 0)


def test_modes_the_shape_does_not_fit_are_refused(host):
    assert plan(host, (6, 6, 18), mode=1)["rc"] == E_LDS and not plan(host, (6, 6, 18), mode=1)["available"]
    assert plan(host, (26, 5, 14), mode=3)["rc"] == E_LDS and not plan(host, (26, 5, 14), mode=3)["available"]
    assert plan(host, (6, 6, 18), mode=3)["rc"] == 0 and plan(host, (6, 6, 18), mode=3)["available"]


def test_failed_workspace_allocation_moves_auto_mode_to_the_lds_kernel(host):
    p = plan(host, (12, 3, 6), gm_ws_failed=True)
    assert (p["kernel"], p["threads"], p["two_sided"], p["soc_lds"], p["lds"], p["inst_off"], p["needs_ws"]) == ("mw r3", 256, 1, 7220, 67648, 6898, 0)
    # ... but not the explicit modes, and not a shape only the workspace kernels hold
    assert plan(host, (12, 3, 6), mode=5, gm_ws_failed=True)["kernel"] == "gm1"
    assert plan(host, (26, 5, 14), gm_ws_failed=True)["kernel"] == "gm"


def test_descriptor_words_of_the_workspace_kernels(host):
    for two_sided in (-1, 0, 1):
        p = plan(host, (12, 3, 6), mode=4, two_sided=two_sided)
        assert (p["kernel"], p["threads"], p["lds"], p["inst_off"], p["soc_lds"], p["needs_ws"]) == ("gm", 256, 17792, 1902, 0, 1)
        assert p["two_sided"] == (1 if two_sided < 0 else two_sided)
        p = plan(host, (12, 3, 6), mode=5, two_sided=two_sided)
        assert (p["kernel"], p["threads"], p["lds"], p["inst_off"], p["soc_lds"], p["two_sided"], p["needs_ws"]) == ("gm1", 64, 17792, 1902, 0, 0, 1)
    # the default sweep: two-sided exactly where the one-wavefront LDS kernels cannot run the shape
    assert plan(host, (5, 3, 6), mode=3)["two_sided"] == 0 and plan(host, (5, 3, 6), mode=3, refused=REFUSED["wave"])["two_sided"] == 1


def test_lds_pad_goes_to_the_one_wavefront_lds_kernels_only(host):
    on = dict(specialise=True, has_wave_shape=True, has_mw_shape=True)
    assert plan(host, (5, 3, 6), lds_pad=4096)["lds"] == 30864 + 4096
    assert plan(host, (5, 3, 6), lds_pad=4096, **on)["lds"] == 30864 + 4096
    assert plan(host, (5, 3, 6), mode=3, lds_pad=4096)["lds"] == 32064
    assert plan(host, (5, 3, 6), mode=4, lds_pad=4096)["lds"] == 9536
    assert plan(host, (5, 3, 6), mode=5, lds_pad=4096)["lds"] == 9536
    assert plan(host, (5, 3, 6), mode=2, lds_pad=4096)["lds"] == 0
    assert plan(host, (20, 5, 14), lds_pad=4096, **on)["lds"] == 161424


def _restated(c, N, nO, mode, spec, has_w, has_mw, two_sided, pad, gm_failed, refused, names):
    """the rule of include/obca_mpc.h on arrays of cases; c: the header's capability numbers per case"""
    fits = lambda nbytes: nbytes + 64 <= 160 * 1024
    wave = (c["R_max"] <= 384) & fits(c["lds_bytes"]) & (refused != REFUSED["wave"])
    mw = (c["R_max"] <= 1280) & fits(c["lds_bytes_mw"]) & (refused != REFUSED["mw"])
    gm = fits(c["lds_bytes_gm"]) & (refused != REFUSED["gm"])
    available = (mode == 0) | (mode == 2) | ((mode == 1) & wave) | ((mode == 3) & mw) | (((mode == 4) | (mode == 5)) & gm)
    auto = mode == 0
    beyond = auto & ~wave
    f_gm1 = (mode == 5) | (beyond & mw & gm & (nO <= 3) & (N <= 26) & ~gm_failed)
    f_gm = (mode == 4) | (beyond & ~mw & gm)
    f_mw = ((mode == 3) | (beyond & mw)) & ~f_gm1
    f_wave = (mode == 1) | (auto & wave)
    f_lane = (mode == 2) | (beyond & ~mw & ~gm)
    assert np.all(f_gm1.astype(int) + f_gm + f_mw + f_wave + f_lane == 1)
    s_mw = f_mw & spec & has_mw & (refused != REFUSED["mw shape"])
    s_w = f_wave & spec & has_w
    R = c["R_max"]
    kernel = np.select([f_gm1, f_gm, s_mw, f_mw & (R <= 768), f_mw, s_w, f_wave & (R <= 256), f_wave & (R <= 320), f_wave, f_lane],
                       [names[k] for k in ("gm1", "gm", "mw shape", "mw r3", "mw r5", "wave shape", "wave r4", "wave r5", "wave r6", "lane")])
    ws = f_gm | f_gm1
    sweep = np.where(two_sided < 0, np.where(wave, 0, 1), two_sided)
    return {"rc": np.where(available, 0, E_LDS), "available": available, "kernel": kernel,
            "threads": np.where(f_mw | f_gm, 256, 64),
            "lds": np.select([ws, f_mw, f_wave], [c["lds_bytes_gm"], c["lds_bytes_mw"], c["lds_bytes"] + pad], 0),
            "inst_off": np.where(ws, c["inst_off_gm"], c["inst_off"]),
            "soc_lds": np.select([ws, f_mw], [0, c["soc_lds_mw"]], c["soc_lds"]),
            "two_sided": np.where(f_gm1, 0, sweep), "needs_ws": ws, "specialised": s_mw | s_w}


def test_plan_agrees_with_the_documented_rule_on_a_sweep(host):
    shapes = []
    for N, nO in itertools.product((1, 5, 6, 12, 20, 26, 27, 40, 74, 127), range(1, 9)):
        for M in sorted({nO, 4 * nO, min(nO, 2) + 4 * max(nO - 2, 0)}):       # every obstacle one edge / four edges / two of one edge, the others four
            shapes.append((N, nO, M))
    # mode, specialise, a wave / a four-wavefront instantiation exists, two_sided, lds_pad (one non-zero value: where it is added),
    # gm_ws_failed, refused (none, each single one)
    knobs = np.array(list(itertools.product(range(6), (0, 1), (0, 1), (0, 1), (-1, 0, 1), (512,), (0, 1), (0, 1, 2, 4, 8))), np.int64)
    cases = np.hstack([np.repeat(np.array(shapes, np.int64), len(knobs), axis=0), np.tile(knobs, (len(shapes), 1))])
    assert len(knobs) == 1440 and len(shapes) >= 10 * 8 * 2
    got = plans(host, cases)
    per_shape = np.array([list(caps(host, *s).values()) for s in shapes], np.int64)
    c = {k: np.repeat(per_shape[:, i], len(knobs)) for i, k in enumerate(CAPS)}
    # the capability flags are the thresholds on the capability numbers
    assert np.array_equal(c["wave_ok"], (c["R_max"] <= 384) & (c["lds_bytes"] + 64 <= 160 * 1024))
    assert np.array_equal(c["mw_ok"], (c["R_max"] <= 1280) & (c["lds_bytes_mw"] + 64 <= 160 * 1024))
    assert np.array_equal(c["gm_ok"], c["lds_bytes_gm"] + 64 <= 160 * 1024)
    names = {host.select_kernel_name(k).decode(): k for k in range(10)}
    assert len(names) == 10 and "?" not in names
    col = lambda i: cases[:, i]
    want = _restated(c, col(0), col(1), col(3), col(4) != 0, col(5) != 0, col(6) != 0, col(7), col(8), col(9) != 0, col(10), names)
    ok = want["available"]
    assert 0 < ok.sum() < len(ok)
    for i, k in enumerate(PLAN):
        sel = slice(None) if k in ("rc", "available") else ok                # a refused plan carries an error, nothing else
        bad = np.flatnonzero((got[:, i] != want[k].astype(np.int64))[sel])
        assert bad.size == 0, (k, cases[sel][bad[0]].tolist(), got[sel][bad[0]].tolist())
    # every branch was reached
    assert set(got[ok, 1].tolist()) == set(range(10))
