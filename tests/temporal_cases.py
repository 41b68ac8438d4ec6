"""The sizes, cameras, guides and chains shared by test_temporal_host.py and test_gpu_temporal.py (test infrastructure; not
a test module). Guides on the CPU are primary_ref.trace of the primary-hit tests' scenes from the moved cameras, computed
once per (scene, move, size) and left unchanged."""
import copy
import functools

import numpy as np

import denoise_cases
import primary_cases
import primary_ref
import wcpt

CPU_SIZES = denoise_cases.CPU_SIZES          # 1x1, 9x5, 37x23
GPU_SIZES = denoise_cases.GPU_SIZES          # + 70x44 (32x8 blocks cut at both edges), 200x120
GUIDES = denoise_cases.GUIDES                # cornell, every_kind, two_draws
# what the camera does between two sequences: nothing, a yaw of 1.5 degrees, a translation, a half-turn
MOVES = ["still", "yaw", "shift", "half_turn"]

image = denoise_cases.image
assert_same_bits = denoise_cases.assert_same_bits
surfaces = denoise_cases.surfaces


def moved_camera(cam, move, steps=1, yaw_step=1.5):
    """A copy of the camera after `steps` moves of the kind `move`."""
    c = copy.copy(cam)
    if move == "yaw":
        c.yaw = cam.yaw + yaw_step * steps
    elif move == "shift":
        for i, d in enumerate((0.05, -0.03, 0.04)):
            c.position[i] = cam.position[i] + d * steps
    elif move == "half_turn":
        c.yaw = cam.yaw + 180.0 * steps
    elif move != "still":
        raise ValueError(move)
    return c


@functools.lru_cache(maxsize=None)
def frame(name, move, width, height, steps=1):
    """(records [height, width], scene data) of scene `name` seen from its camera after the move (read-only, shared)."""
    s = primary_cases.scene(name)
    sd = s.scene_data(width, height, max_bounce=0, samples=1, frame=0, camera=moved_camera(s.camera, move, steps))
    if move == "still":
        rec = primary_ref.reference(name, s, width, height)[0]
    else:
        rec = primary_ref.trace(s, width, height, sd=sd)[0]
        rec.setflags(write=False)
    sd.setflags(write=False)
    return rec, sd


def chain(name, move, width, height, kind):
    """The three calls of the CPU chain as (image, frames, restart, records, scene data): a restart without history, a call
    that is no restart with two frames accumulated, a restart after the move."""
    rec0, sd0 = frame(name, "still", width, height)
    rec1, sd1 = frame(name, move, width, height)
    img0 = image(width, height, kind)
    img1 = (img0 * np.float32(0.75) + np.float32(0.125)).astype(np.float32)     # the grown accumulation image
    other = "noise" if kind == "special" else "special"
    img2 = image(width, height, other)[::-1, ::-1].copy()                         # another image for the new sequence
    return [(img0, 1, True, rec0, sd0), (img1, 2, False, rec0, sd0), (img2, 1, True, rec1, sd1)]


def run_chain(calls, step, params=None):
    """The states after each call of `calls`, each made by step(img, frames, rec, sd, restart, history, state) -> (base,
    n_b, rgba, length): the bookkeeping a caller of the stateless twin does."""
    out = []
    history = None          # (rgba, length, records, sd) of the last call, with the sequence's records and scene data
    state = None
    seq = None
    for img, frames, restart, rec, sd in calls:
        if restart or history is None:
            base, n_b, rgba, length = step(img, frames, rec, sd, True, history, None)
            seq = (rec, sd)
        else:
            base, n_b, rgba, length = step(img, frames, rec, sd, False, None, state)
        state = (base, n_b)
        history = (rgba, length, seq[0], seq[1])
        out.append((base, n_b, rgba, length))
    return out


def host_step(params):
    def step(img, frames, rec, sd, restart, history, state):
        return wcpt.temporal_host(img, frames, rec, sd, params, restart=restart, history=history, state=state)
    return step
