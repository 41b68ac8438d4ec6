"""Temporal reprojection on the CPU (no GPU): wcpt_temporal_host, the host build of csrc/wcpt_temporal.h, against the
independent numpy restatement in temporal_ref.py bit for bit over chains of calls, the rule's exact properties, the round trip
of an unmoved camera, what the stage is worth against the oracle's converged frames, the refusals, the ABI layout, and the
header's host loop under AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program
(tests/temporal_asan_driver.cpp)."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle
import primary_cases
import primary_ref
import temporal_cases as tc
import temporal_ref
import wcpt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = wcpt._lib.WCPT_ERROR_INVALID_ARGUMENT
T = wcpt._lib
F = np.float32


def ref_step(params):
    def step(img, frames, rec, sd, restart, history, state):
        return temporal_ref.call(img, frames, rec, sd, restart, history, state, params.max_history, params.normal_min,
                                 params.depth_tol)
    return step


def assert_states_equal(got, ref, what):
    for i, (g, r) in enumerate(zip(got, ref)):
        for name, a, b in zip(("base", "n_b", "rgba", "length"), g, r):
            assert a.shape == b.shape, (what, i, name)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, "call", i, name)


# ---- the numpy restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["noise", "special"])
@pytest.mark.parametrize("move", tc.MOVES)
@pytest.mark.parametrize("name", tc.GUIDES)
@pytest.mark.parametrize("size", tc.CPU_SIZES, ids=lambda s: "%dx%d" % s)
def test_temporal_host_matches_reference(size, name, move, kind):
    """wcpt_temporal_host equals the numpy restatement bit for bit in all four outputs after each call of a chain: a restart
    without history, a call that is no restart with two frames, a restart with the camera moved -- HDR noise, and noise
    with 0, 25, NaN, inf and negative values in the image and so in the history (NaN positions must agree)."""
    calls = tc.chain(name, move, *size, kind)
    p = wcpt.TemporalParams()
    got = tc.run_chain(calls, tc.host_step(p))
    assert_states_equal(got, tc.run_chain(calls, ref_step(p)), (size, name, move, kind))
    # the chain does what it is there for: the second call re-blends, the third finds history unless the camera turned away
    if size != (1, 1):
        assert (got[2][1] > 0).any() == (move != "half_turn")
        assert (got[1][3] == 2.0).all() and (got[0][3] == 1.0).all()


def test_parameters_reach_the_arithmetic():
    """Each parameter equals the restatement with the same value and differs from the defaults' result."""
    size = (37, 23)
    calls = tc.chain("cornell", "yaw", *size, "noise")
    base = tc.run_chain(calls, tc.host_step(wcpt.TemporalParams()))
    for p in [wcpt.TemporalParams(1), wcpt.TemporalParams(32, 0.99999), wcpt.TemporalParams(32, 0.9, 0.0005),
              wcpt.TemporalParams(65536, -1.0, 1.0e3)]:
        got = tc.run_chain(calls, tc.host_step(p))
        assert_states_equal(got, tc.run_chain(calls, ref_step(p)), (p.max_history, p.normal_min, p.depth_tol))
        assert any(not np.array_equal(a, b, equal_nan=True) for a, b in zip(got[2], base[2]))


# ---- exact properties ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.GUIDES)
def test_half_turn_finds_no_history(name):
    """After a half-turn nothing of the old frame is in front of the camera: every carried length n_b is 0 and the output
    is the accumulation image bit for bit."""
    W, H = 37, 23
    calls = tc.chain(name, "half_turn", W, H, "noise")
    base, n_b, rgba, length = tc.run_chain(calls, tc.host_step(wcpt.TemporalParams()))[2]
    assert (n_b == 0).all() and (base.view(np.uint32) == 0).all()
    assert np.array_equal(rgba.view(np.uint32), calls[2][0].view(np.uint32))
    assert (length == 1.0).all()


@pytest.mark.parametrize("name", ["every_kind", "cornell"])
def test_nothing_leaks_across_an_identity(name):
    """A history that is 1.0 on one identity and +0.0 on another: after a small move base is exactly +0.0 on every pixel of
    the second identity, for the largest surfaces of the frame."""
    W, H = tc.denoise_cases.PROPERTY_SIZE
    rec0, sd0 = tc.frame(name, "still", W, H)
    rec1, sd1 = tc.frame(name, "yaw", W, H)
    ids0, ids1 = tc.surfaces(rec0), tc.surfaces(rec1)
    values, counts = np.unique(ids1, return_counts=True)
    checked = 0
    for v in values[np.argsort(-counts)][:4]:
        hist = np.ones((H, W, 4), F)
        hist[ids0 == v, :3] = 0.0
        length = np.full((H, W), 3.0, F)
        cur = np.full((H, W, 4), 0.5, F)
        base, n_b, _, _ = wcpt.temporal_host(cur, 1, rec1, sd1, history=(hist, length, rec0, sd0))
        mask = ids1 == v
        assert (n_b[mask] > 0).sum() > 0.5 * mask.sum()            # the surface does find its history
        assert (base[mask].view(np.uint32) == 0).all()             # and nothing but its own
        other = ~mask & (n_b > 0)
        assert other.any() and (base[other] == 1.0).all()
        checked += 1
    assert checked >= 3


def test_length_never_exceeds_max_history():
    """40 restarts with a still camera: every stored length is at most max_history, and reaches it."""
    W, H = 9, 5
    rec, sd = tc.frame("cornell", "still", W, H)
    p = wcpt.TemporalParams(7)
    img = tc.image(W, H, "noise")
    history = None
    for i in range(40):
        base, n_b, rgba, length = wcpt.temporal_host(img, 1, rec, sd, p, history=history)
        assert (length <= 7.0).all() and (length >= 1.0).all()
        assert (length == np.minimum(n_b + F(1.0), F(7.0))).all()
        history = (rgba, length, rec, sd)
    assert (length == 7.0).all()


def test_nan_history_is_gone_after_one_restart():
    """A NaN texel of the history does not count as a tap: the sequence after the restart holds no NaN."""
    W, H = 37, 23
    rec, sd = tc.frame("cornell", "still", W, H)
    rec1, sd1 = tc.frame("cornell", "yaw", W, H)
    img = tc.image(W, H, "noise")
    bad = img.copy()
    bad[5:9, 7:12, 0] = np.nan
    bad[12, 3, 1] = np.inf
    _, _, rgba, length = wcpt.temporal_host(bad, 1, rec, sd)
    assert np.isnan(rgba).any()
    for r, s in [(rec, sd), (rec1, sd1)]:
        base, n_b, out, _ = wcpt.temporal_host(img, 1, r, s, history=(rgba, length, rec, sd))
        assert np.isfinite(base).all() and np.isfinite(out).all() and (n_b > 0).any()


# ---- round trip --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(70, 44), (200, 120)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", tc.GUIDES)
def test_unmoved_camera_reprojects_every_hit_onto_itself(name, size):
    """With the camera unmoved every hit pixel comes back to within 0.01 pixel of its own centre (the error is a few dozen
    ulps of a coordinate below 256, about 1e-3): in the restatement's positions, which the parity test pins to the
    library bit for bit, and in the library itself, whose base of a history that holds each texel's coordinates is then
    that coordinate."""
    W, H = size
    rec, sd = tc.frame(name, "still", W, H)
    hit = (rec["kind"] & 3) != 0
    assert hit.sum() > 0.3 * W * H
    valid, fx, fy = temporal_ref.positions(rec, np.asarray(sd["position"], F), temporal_ref.camera(sd, W, H), W, H)
    ys, xs = np.mgrid[0:H, 0:W]
    assert valid[hit].all()
    ex, ey = np.abs(fx - xs)[hit].max(), np.abs(fy - ys)[hit].max()
    print(f"{name} {W}x{H}: max |fx - x| {ex:.3g}, max |fy - y| {ey:.3g}")
    assert ex <= 0.01 and ey <= 0.01
    coords = np.zeros((H, W, 4), F)
    coords[..., 0], coords[..., 1] = xs, ys
    base, n_b, _, _ = wcpt.temporal_host(coords, 1, rec, sd, history=(coords, np.ones((H, W), F), rec, sd))
    assert (n_b[hit] > 0).all()
    assert np.abs(base[..., 0] - xs)[hit].max() <= 0.01 and np.abs(base[..., 1] - ys)[hit].max() <= 0.01


# ---- what it is worth --------------------------------------------------------------------------------------------------------
def _display_rgb(img):
    return np.clip(oracle.composite(img)[0][..., :3].astype(np.float64), 0.0, 1.0)


@functools.lru_cache(maxsize=None)
def _quality(name, yaw_step):
    """(err raw, err temporal, err temporal + default denoise) of the last of eight one-sample frames, the camera yawing
    yaw_step degrees a frame, against the oracle's 1024-sample frame at the last camera."""
    W, H = 96, 64
    s = primary_cases.get_scene(name)
    history = None
    for i in range(8):
        cam = tc.moved_camera(s.camera, "yaw", i, yaw_step)
        sd = s.scene_data(W, H, max_bounce=4, samples=1, frame=0, camera=cam)
        raw = oracle.render_scene(s, W, H, sd=sd)[0]
        rec = primary_ref.trace(s, W, H, sd=sd)[0]
        _, _, out, length = wcpt.temporal_host(raw, 1, rec, sd, history=history)
        history = (out, length, rec, sd)
    sdc = s.scene_data(W, H, max_bounce=4, samples=1024, frame=0, camera=cam)
    conv = oracle.render_scene(s, W, H, sd=sdc, threads=min(16, os.cpu_count() or 1))[0]
    want = _display_rgb(conv)
    den = wcpt.denoise_host(out, rec)[0]          # already the display value: clip it as the others
    return (float(np.mean((_display_rgb(raw) - want) ** 2)), float(np.mean((_display_rgb(out) - want) ** 2)),
            float(np.mean((np.clip(den[..., :3].astype(np.float64), 0.0, 1.0) - want) ** 2)))


@pytest.mark.parametrize("name", ["cornell", "reference_init"])
def test_temporal_halves_the_display_error(name):
    """96x64, max_bounce 4, eight one-sample frames (each frame 0) with the camera yawing 1.5 degrees a frame, about 1.6
    pixels: the mean squared display-space error of the temporal output at the last frame against the oracle's 1024-sample
    frame there is at most half the raw frame's. Measured with this build (error ratios to the raw frame's):
      cornell         1.5 degrees: temporal 0.082 (0.00767 against 0.0931), then the default denoise 0.037
                      0.2 degrees: temporal 0.300, then the default denoise 0.040
      reference_init  1.5 degrees: temporal 0.025 (0.000320 against 0.01260), then the default denoise 0.052
                      0.2 degrees: temporal 0.131, then the default denoise 0.050
    The 0.2-degree step is the sub-pixel case: a restarted frame's seed is the same for a pixel in every frame, so history
    that arrives from the same pixel adds little. Those and the denoised figures are printed, not
    asserted."""
    err_raw, err_t, err_td = _quality(name, 1.5)
    print(f"{name} 1.5 deg: err(raw) {err_raw:.6g} err(temporal) {err_t:.6g} ratio {err_t / err_raw:.4f} "
          f"err(temporal+denoise) {err_td:.6g} ratio {err_td / err_raw:.4f}")
    sub_raw, sub_t, sub_td = _quality(name, 0.2)
    print(f"{name} 0.2 deg: err(raw) {sub_raw:.6g} err(temporal) {sub_t:.6g} ratio {sub_t / sub_raw:.4f} "
          f"err(temporal+denoise) {sub_td:.6g} ratio {sub_td / sub_raw:.4f}")
    assert err_t <= 0.5 * err_raw


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _singular(sd, field):
    bad = sd.copy()
    m = np.asarray(bad[field]).copy().reshape(4, 4)
    m[1] = m[0]                                   # two equal columns
    bad[field] = m.reshape(16)
    return bad


def _orthographic(sd):
    bad = sd.copy()
    proj = np.diag([0.5, 0.5, -0.01, 1.0])
    proj[2, 3] = -1.0                             # an orthographic projection: w does not depend on the point
    bad["inverseProjection"] = np.linalg.inv(proj).T.reshape(16).astype(F)
    return bad


REFUSALS = ["null params", "null image", "null guide", "null scene", "null base", "null n_b", "null out", "null length",
            "frames 0", "max_history 0", "max_history 65537", "normal_min nan", "normal_min > 1", "normal_min < -1",
            "depth_tol 0", "depth_tol < 0", "depth_tol inf", "depth_tol nan", "width 0", "height 0",
            "singular inverseProjection", "singular inverseView", "nan matrix", "orthographic", "singular history camera",
            "history without lengths", "history without scene"]


@pytest.mark.parametrize("what", REFUSALS)
def test_temporal_host_refusals(what):
    """Every refusal returns WCPT_ERROR_INVALID_ARGUMENT and leaves all four outputs untouched."""
    W, H = 9, 5
    img = tc.image(W, H, "noise")
    rec, sd = tc.frame("cornell", "still", W, H)
    rec, sd = np.ascontiguousarray(rec), np.ascontiguousarray(sd)
    nan, inf = float("nan"), float("inf")
    p = {"max_history 0": wcpt.TemporalParams(0), "max_history 65537": wcpt.TemporalParams(65537),
         "normal_min nan": wcpt.TemporalParams(32, nan), "normal_min > 1": wcpt.TemporalParams(32, 1.5),
         "normal_min < -1": wcpt.TemporalParams(32, -1.5), "depth_tol 0": wcpt.TemporalParams(32, 0.9, 0.0),
         "depth_tol < 0": wcpt.TemporalParams(32, 0.9, -0.05), "depth_tol inf": wcpt.TemporalParams(32, 0.9, inf),
         "depth_tol nan": wcpt.TemporalParams(32, 0.9, nan)}.get(what, wcpt.TemporalParams())
    scene = sd
    if what == "singular inverseProjection":
        scene = _singular(sd, "inverseProjection")
    elif what == "singular inverseView":
        scene = _singular(sd, "inverseView")
    elif what == "nan matrix":
        scene = sd.copy()
        scene["inverseView"][..., 5] = nan
    elif what == "orthographic":
        scene = _orthographic(sd)
    hist_img, hist_len, hist_sd = img.copy(), np.ones((H, W), F), sd
    if what == "singular history camera":
        hist_sd = _singular(sd, "inverseProjection")
    base = np.full((H, W, 3), -7.0, F)
    n_b = np.full((H, W), -7.0, F)
    out = np.full((H, W, 4), -7.0, F)
    length = np.full((H, W), -7.0, F)

    def arg(name, a):
        return None if what == name else a.ctypes.data

    rc = wcpt.lib.wcpt_temporal_host(
        arg("null image", img), 0 if what == "frames 0" else 1, 1, arg("null guide", rec), arg("null scene", scene),
        0 if what == "width 0" else W, 0 if what == "height 0" else H, None if what == "null params" else C.byref(p),
        hist_img.ctypes.data, arg("history without lengths", hist_len), rec.ctypes.data, arg("history without scene", hist_sd),
        arg("null base", base), arg("null n_b", n_b), arg("null out", out), arg("null length", length))
    assert rc == INVALID
    assert (base == -7.0).all() and (n_b == -7.0).all() and (out == -7.0).all() and (length == -7.0).all()
    if what.startswith(("max_history", "normal_min", "depth_tol")):
        with pytest.raises(wcpt.WcptError):
            wcpt.temporal_host(img, 1, rec, sd, p)
    # the same call with valid arguments succeeds, the extreme parameters included
    good = wcpt.TemporalParams(65536, -1.0, 1.0e30)
    assert wcpt.lib.wcpt_temporal_host(img.ctypes.data, 1, 1, rec.ctypes.data, sd.ctypes.data, W, H, C.byref(good),
                                       hist_img.ctypes.data, hist_len.ctypes.data, rec.ctypes.data, sd.ctypes.data,
                                       base.ctypes.data, n_b.ctypes.data, out.ctypes.data, length.ctypes.data) == 0
    assert (n_b > 0).any()


def test_the_restatement_refuses_the_same_cameras():
    W, H = 9, 5
    sd = np.ascontiguousarray(tc.frame("cornell", "still", W, H)[1])
    assert temporal_ref.camera(sd, W, H) is not None
    for bad in (_singular(sd, "inverseProjection"), _singular(sd, "inverseView"), _orthographic(sd)):
        assert temporal_ref.camera(bad, W, H) is None


def test_python_wrappers_check_their_arguments():
    """Context.composite's own refusals need no device: they are raised before the first call into the library."""
    ctx = wcpt.Context.__new__(wcpt.Context)
    ctx.h = None
    ctx.owned = False
    t = wcpt.TemporalParams()
    sd = tc.frame("cornell", "still", 9, 5)[1]
    with pytest.raises(ValueError):
        ctx.composite(16, temporal=t, scene=sd, frames=1)                                  # no guide
    with pytest.raises(ValueError):
        ctx.composite(16, temporal=t, guide=16, frames=1)                                  # no scene
    with pytest.raises(ValueError):
        ctx.composite(16, temporal=t, guide=16, scene=sd)                                  # no frame count
    with pytest.raises(ValueError):
        ctx.composite(16, temporal=t, guide=16, scene=sd, frames=1, bloom=wcpt.BloomParams())
    with pytest.raises(ValueError):
        wcpt.temporal_host(np.zeros((5, 9, 4), F), 1, np.zeros((5, 8), T.PRIMARY_HIT_DTYPE), sd)
    with pytest.raises(ValueError):
        wcpt.temporal_host(np.zeros((5, 9, 4), F), 2, np.zeros((5, 9), T.PRIMARY_HIT_DTYPE), sd, restart=False)
    assert wcpt.lib.wcpt_composite_temporal(None, None, 1, 1, 16, 48, 16, 0, None, None) == T.WCPT_ERROR_INVALID_HANDLE
    assert wcpt.lib.wcpt_temporal_reset(None) == T.WCPT_ERROR_INVALID_HANDLE


# ---- ABI layout --------------------------------------------------------------------------------------------------------------
def test_temporal_params_layout(tmp_path):
    """sizeof(wcpt_temporal_params) == 16 and its field offsets, in C and in the ctypes mirror, whose defaults are the
    header's."""
    header = os.path.join(ROOT, "include", "wcpt.h")
    src = tmp_path / "t.c"
    src.write_text(f'''#include "{header}"
#include <stddef.h>
_Static_assert(sizeof(wcpt_temporal_params) == 16, "wcpt_temporal_params");
_Static_assert(offsetof(wcpt_temporal_params, max_history) == 0 && offsetof(wcpt_temporal_params, normal_min) == 4, "fields");
_Static_assert(offsetof(wcpt_temporal_params, depth_tol) == 8 && offsetof(wcpt_temporal_params, _pad) == 12, "fields");
int main(void) {{ return 0; }}
''')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", str(src), "-o", str(tmp_path / "t.o")], check=True)
    P = wcpt.TemporalParams
    assert C.sizeof(P) == 16
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [("max_history", 0), ("normal_min", 4), ("depth_tol", 8),
                                                                  ("_pad", 12)]
    p = P()
    assert p.max_history == 32 and p.normal_min == F(0.9) and p.depth_tol == F(0.05) and p._pad == 0
    text = open(header).read()
    assert re.search(r"Callers' defaults: 32, 0\.9, 0\.05\.", text)


# ---- sanitizers --------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_temporal_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "temporal_asan_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-ffp-contract=off",
           os.path.join(ROOT, "tests", "temporal_asan_driver.cpp"),
           os.path.join(ROOT, "wc-path-tracer_amd", "host", "wcpt_host.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "0 failed checks" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
