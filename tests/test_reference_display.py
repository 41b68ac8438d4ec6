"""The display step against the reference's own composite.comp and bloom.comp, executed (oracle/refshader.py): the oracle's
composite, tests/bloom_ref.py's numpy restatement and the product's wcpt_bloom_host, bit for bit on every texel (a NaN must
meet a NaN). The reference has no host code that dispatches bloom.comp; the chain is the protocol of DESIGN.md §8."""
import numpy as np
import pytest

import bloom_cases
import bloom_ref
import oracle
import ref_cases
import refshader
import wcpt
from ref_cases import assert_same_bits

F = np.float32


@pytest.fixture(scope="module")
def ref():
    return ref_cases.reference_library()


def rgba(rgb):
    """a float4 level from an RGB one (the shaders store alpha 1)"""
    out = np.ones(rgb.shape[:2] + (4,), F)
    out[..., :3] = rgb
    return out


def test_composite_matches_oracle(ref):
    """composite.comp without Bloom on the synthetic HDR set (0, 1, NaN, inf, negative, every tonemap branch) and on a
    rendered frame, at a width and height that are no powers of two."""
    hdr = ref_cases.hdr_image()
    for src in (hdr, ref_cases.oracle_result("cornell")[0], bloom_cases.image(37, 23, "special")):
        assert_same_bits(ref.composite(src), oracle.composite(src)[0], "composite")
    out = ref.composite(hdr)
    assert np.isnan(out[0, 2, 0]) and (out[..., 3] == 1.0).all()
    peak = out[..., :3].max(axis=2)
    assert (peak[1:] < 0.76).any() and (peak[1:] > 0.76).any()          # below and above startCompression


@pytest.mark.parametrize("size", [(36, 20), (7, 5), (1, 1)], ids=lambda s: "%dx%d" % s)
def test_composite_with_a_bloom_texture(ref, size):
    """The Bloom branch (composite.comp:45-46): the image's texel plus the linear sample of a smaller bloom texture."""
    hdr = ref_cases.hdr_image()
    rng = np.random.default_rng(5)
    bloom = rgba((rng.random((size[1], size[0], 3)) * 3.0).astype(F))
    bloom[0, 0, :3] = [np.inf, 0.0, -1.0]
    u, v = bloom_ref.texel_coords(hdr.shape[1], hdr.shape[0])
    with np.errstate(all="ignore"):
        s = hdr.copy()
        s[..., :3] = hdr[..., :3] + bloom_ref.sample(bloom[..., :3], u, v)
    assert_same_bits(ref.composite(hdr, bloom=bloom), oracle.composite(s)[0], "composite with Bloom")
    assert not np.array_equal(ref.composite(hdr, bloom=bloom)[1:], ref.composite(hdr)[1:])


@pytest.mark.parametrize("kind", ["noise", "special"])
@pytest.mark.parametrize("size", [(16, 16), (37, 23), (9, 5)], ids=lambda s: "%dx%d" % s)
def test_bloom_modes_one_dispatch_each(ref, size, kind):
    """bloom.comp one dispatch per Mode against bloom_ref.box13, prefilter and tent9, with the level read at a LOD > 0
    where the Mode takes one."""
    img = bloom_cases.image(*size, kind)
    (w0, h0), (w1, h1) = bloom_ref.level_sizes(*size, 2)
    params = ref_cases.bloom_params()
    rng = np.random.default_rng(6)
    with np.errstate(all="ignore"):
        u0, v0 = bloom_ref.texel_coords(w0, h0)
        u1, v1 = bloom_ref.texel_coords(w1, h1)
        want = bloom_ref.prefilter(bloom_ref.box13(img[..., :3], u0, v0), params)
        got = ref.bloom_dispatch(refshader.MODE_PREFILTER, params, 0, [img], None, w0, h0)
        assert_same_bits(np.ascontiguousarray(got[..., :3]), want, "MODE_PREFILTER")
        assert (got[..., 3] == 1.0).all()
        # MODE_DOWNSAMPLE reading level 1 of a texture whose level 0 is something else
        src = rgba((rng.random((h0, w0, 3)) * 4.0).astype(F))
        src[0, 0, :3] = img[1, 2, :3] if kind == "special" else 0.0        # a NaN texel in the special set
        decoy = rgba(np.full((size[1], size[0], 3), 7.0, F))
        got = ref.bloom_dispatch(refshader.MODE_DOWNSAMPLE, params, 1, [decoy, src], None, w1, h1)
        assert_same_bits(np.ascontiguousarray(got[..., :3]), bloom_ref.box13(src[..., :3], u1, v1), "MODE_DOWNSAMPLE")
        # MODE_UPSAMPLE_FIRST: D[0] + Tent9(D[1]); MODE_UPSAMPLE: D[0] + Tent9(U[1]) from the other texture
        d0 = rgba((rng.random((h0, w0, 3)) * 2.0).astype(F))
        d1 = rgba((rng.random((h1, w1, 3)) * 2.0).astype(F))
        up1 = rgba((rng.random((h1, w1, 3)) * 2.0).astype(F))
        got = ref.bloom_dispatch(refshader.MODE_UPSAMPLE_FIRST, params, 0, [d0, d1], None, w0, h0)
        assert_same_bits(np.ascontiguousarray(got[..., :3]), d0[..., :3] + bloom_ref.tent9(d1[..., :3], u0, v0),
                         "MODE_UPSAMPLE_FIRST")
        got = ref.bloom_dispatch(refshader.MODE_UPSAMPLE, params, 0, [d0, d1], [None, up1], w0, h0)
        assert_same_bits(np.ascontiguousarray(got[..., :3]), d0[..., :3] + bloom_ref.tent9(up1[..., :3], u0, v0),
                         "MODE_UPSAMPLE")


@pytest.mark.parametrize("kind", bloom_cases.INPUTS)
@pytest.mark.parametrize("size", bloom_cases.SIZES, ids=lambda s: "%dx%d" % s)
def test_bloom_chain(ref, size, kind):
    """The whole chain through the compiled shaders against bloom_ref.pyramid (the texture composite.comp samples) and
    against wcpt_bloom_host (the displayed image): odd sizes and one-texel levels included."""
    img = bloom_cases.image(*size, kind)
    sizes = bloom_ref.level_sizes(*size, 6)
    assert sizes == wcpt.bloom_levels(*size, 6)
    _, up, display = ref_cases.reference_bloom_chain(ref, img, sizes)
    assert_same_bits(np.ascontiguousarray(up[0][..., :3]), bloom_ref.pyramid(img), "U[0]")
    assert_same_bits(display, wcpt.bloom_host(img)[0], "wcpt_bloom_host")


def test_bloom_chain_with_other_parameters(ref):
    img = bloom_cases.image(37, 23, "noise")
    for threshold, knee, levels in [(2.5, 0.1, 6), (1.0, 0.75, 6), (1.0, 0.1, 2), (0.0, 0.001, 3)]:
        sizes = bloom_ref.level_sizes(37, 23, levels)
        _, up, display = ref_cases.reference_bloom_chain(ref, img, sizes, threshold, knee)
        assert_same_bits(np.ascontiguousarray(up[0][..., :3]), bloom_ref.pyramid(img, threshold, knee, levels), "U[0]")
        assert_same_bits(display, wcpt.bloom_host(img, wcpt.BloomParams(threshold, knee, levels))[0], "wcpt_bloom_host")
