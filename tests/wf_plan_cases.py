"""A second statement of the wavefront launch rules, for tests/test_wf_plan.py: plain Python written from the text of
launch_wavefront, pipe_begin, pipe_iterate, wf_geo, wf_trace_geo and the two dispatch ladders as they stood in
pt_wavefront.hip before wc-path-tracer_amd/csrc/wf_plan.h took them over. It shares nothing with the header; the
constants are the build switches' defaults. Python integers do not wrap, and the sweep stays where none of the old
32-bit expressions did.
"""
import itertools
import random

RENDER, COUNT, DIAG = 0, 1, 2
MAX_PIPES = 4
FETCH_ONCE_RATIO = 8       # WCPT_WF_FETCH_ONCE_RATIO
SHADE_BLOCKS_PER_CU = 4    # WCPT_SHADE_BLOCKS_PER_CU
PERSIST_GEO = 3            # WCPT_WF_PERSIST_GEO

# the twelve wf_trace instances of a code object: (count, diag, geo, ldsn, persist)
BUILT = {
    (0, 0, 0, 10, 0), (0, 0, 1, 10, 0), (0, 0, 1, 16, 0), (0, 0, 1, 24, 0), (0, 0, 2, 10, 0), (0, 0, 3, 10, 0),
    (1, 0, 0, 10, 0), (1, 0, 1, 10, 0),
    (1, 1, 0, 10, 0), (1, 1, 1, 10, 0),
    (0, 0, 2, 10, 1), (0, 0, 3, 10, 1),
}


def old_geo(mode, draws, fast, ldsn):
    if draws != 1:
        return 0
    return 2 if (fast and mode == RENDER and ldsn == 10) else 1


def old_dispatch(mode, geo, ldsn):
    """the instance the old if-ladder launched for (mode, geo, ldsn)"""
    single = geo >= 1
    if mode == COUNT:
        return (1, 0, 1 if single else 0, 10, 0)
    if mode == DIAG:
        return (1, 1, 1 if single else 0, 10, 0)
    if not single:
        return (0, 0, 0, 10, 0)
    if geo == 2:
        return (0, 0, 2, 10, 0)
    if geo == 3:
        return (0, 0, 3, 10, 0)
    if ldsn == 16:
        return (0, 0, 1, 16, 0)
    if ldsn == 24:
        return (0, 0, 1, 24, 0)
    return (0, 0, 1, 10, 0)


def select(mode, draws, fast, lds_stack):
    """the instance whose occupancy sized the trace grid"""
    ldsn = lds_stack if lds_stack in (16, 24) else 10
    return old_dispatch(mode, old_geo(mode, draws, fast, ldsn), ldsn)


def plan(mode, draws, fast, lds_stack, W, rows, samples, max_bounce, wf_fetch, wf_persist, pipes, sort, overlap, cus,
         trace_bpc, persist_bpc):
    """launch_wavefront up to its first HIP call after the occupancy queries, then each pipeline's pipe_begin and
    pipe_iterate numbers"""
    tiles_x, tiles_y = (W + 7) // 8, (rows + 7) // 8
    total64 = tiles_x * tiles_y * 64
    out = dict(ok=True, empty=False, persist=False, W=W, rows=rows, K=0, trace_grid=0, shade_grid=0, persist_grid=0, pipe=[])
    if total64 == 0:
        out["empty"] = True
        return out
    if total64 > 0xFFFFFFC0 or W * rows > 0xFFFFFFFF:
        out["ok"] = False
        return out
    ldsn = lds_stack if lds_stack in (16, 24) else 10
    geo = old_geo(mode, draws, fast, ldsn)
    trace_grid = trace_bpc * cus
    out["shade_grid"] = cus * SHADE_BLOCKS_PER_CU
    sort = bool(sort) and draws > 0
    persist_ok = mode == RENDER and geo == 2 and samples == 1 and not sort and wf_persist != 0
    persist_full = persist_bpc * cus if persist_ok else 0
    persist = persist_ok and (wf_persist > 0 or W * rows * 5 <= 64 * 7 * persist_full)
    K = min(pipes, MAX_PIPES)
    if pipes < 1:
        if persist:
            K = 2 if (overlap != 0 and mode == RENDER) else 1
        else:
            K = 3 if W * rows <= FETCH_ONCE_RATIO * 64 * trace_grid else 2
    if sort or mode == DIAG:
        K = 1
    tiles = tiles_x * tiles_y
    K = min(K, tiles)
    if K > 1:
        trace_grid = max(trace_grid // K, 1)
    persist_grid = max(1, persist_full // K) if persist else 0
    out.update(persist=persist, K=K, trace_grid=trace_grid, persist_grid=persist_grid)
    for pipe in range(K):
        # pipe_begin
        total = ((tiles - pipe + K - 1) // K) * 64
        P = min(total, W * rows)
        init_grid = min((total + 255) // 256, cus * 16)
        # pipe_iterate
        g = geo
        if geo == 2 and wf_fetch != 0:
            g = 3 if (wf_fetch > 0 or P <= FETCH_ONCE_RATIO * 64 * trace_grid) else 2
        iters = samples * (max_bounce + 1)
        if mode == RENDER and samples > 1:
            iters = max_bounce + 1 + (samples - 1) * max_bounce
        iters = min(iters, 1 << 20)
        variant = (0, 0, PERSIST_GEO, 10, 1) if persist else old_dispatch(mode, g, ldsn)
        out["pipe"].append(dict(tiles=total // 64, total=total, paths=P, init_grid=init_grid,
                                geo=PERSIST_GEO if persist else g, iters=iters, variant=variant))
    return out


def continues(p, mode, overlap, pending, pending_pipes, pending_w, pending_rows, pending_persist):
    return bool(overlap != 0 and p["K"] > 1 and mode == RENDER and pending and pending_pipes == p["K"] and
                pending_w == p["W"] and pending_rows == p["rows"] and bool(pending_persist) == (p["persist_grid"] != 0))


# the sweep: frames below a tile, off the tile grid, row blocks, 1080p and 4K
FRAMES = ((1, 1), (7, 5), (8, 8), (9, 8), (13, 17), (64, 64), (100, 75), (640, 360), (1920, 8), (1920, 135), (1920, 136),
          (1920, 180), (1920, 216), (1920, 270), (1920, 1080), (3840, 2160))
OCCUPANCY = ((32, 16), (8, 4), (1, 1))   # (trace, persistent) blocks per CU
CUS = (256, 64, 1)
OPTION_SETS_PER_FRAME = 8


def sweep():
    """(keyword arguments of plan) over every frame x mode x draw count x layout x occupancy x CU count, each with a few
    option sets drawn from a fixed-seed generator"""
    rng = random.Random(20240917)
    for (W, rows), mode, draws, fast, (tb, pb), cus in itertools.product(FRAMES, (RENDER, COUNT, DIAG), (0, 1, 2), (0, 1),
                                                                         OCCUPANCY, CUS):
        for _ in range(OPTION_SETS_PER_FRAME):
            yield dict(mode=mode, draws=draws, fast=fast, lds_stack=rng.choice((0, 10, 16, 24, 7)), W=W, rows=rows,
                       samples=rng.choice((1, 1, 1, 2, 5)), max_bounce=rng.choice((0, 1, 4, 8)),
                       wf_fetch=rng.choice((-1, -1, 0, 1)), wf_persist=rng.choice((-1, -1, 0, 1)),
                       pipes=rng.choice((0, 0, 1, 2, 3, 4, 5, 9, -1)), sort=rng.choice((0, 0, 1)),
                       overlap=rng.choice((0, 1, 2)), cus=cus, trace_bpc=tb, persist_bpc=pb)
