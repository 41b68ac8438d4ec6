"""The C oracle against the reference's own pathTracer.comp, executed: the shader text is translated mechanically
(oracle/ref_translate.py), compiled for the CPU behind oracle/glsl_cpu.hpp and called through oracle/refshader.py.

Every comparison is of bit patterns, over every channel of every pixel, with no tolerance and no share left out; a NaN
must sit in the same place on both sides (payloads are not compared).

The stack guard. The shader's `uint nodeStack[32]` is a real array in the compiled reference, so before any call into it
the oracle's counters must say ref_stack_max <= 32 and ref_stack_overflow_segments == 0 for the case. Dropped by that
guard: deep_chain_40 and deep_chain_33 (tests/deep_tree.py's hand-made chains, deeper than the stack by construction).
Checked and kept: the atrium (27 levels; deepest stack 23 at 48x32, 4 bounces) and every other case of tests/ref_cases.py.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import golden_cases
import oracle
import ref_cases
import refshader

ORACLE_DIR = os.path.dirname(os.path.abspath(refshader.__file__))


@pytest.fixture(scope="module")
def ref():
    return ref_cases.reference_library()


def test_build_left_the_translate_report(ref):
    """build() leaves the list of rewritten lines beside the library, and nothing translated outside oracle/_ref/."""
    with open(refshader.REPORT_PATH, encoding="utf-8") as f:
        head = f.readline().split()
    assert head[1:3] == ["files", "translated,"] and int(head[0]) >= 3 and int(head[3]) > 0
    if shutil.which("git"):
        tracked = subprocess.run(["git", "ls-files", "oracle/_ref"], cwd=os.path.dirname(ORACLE_DIR), capture_output=True,
                                 text=True)
        assert tracked.returncode != 0 or tracked.stdout.strip() == ""


def test_translator_names_no_identifier_of_the_shaders(ref):
    """Every identifier in the rewritten declarations (block, member, global and parameter names, main's new names) comes
    from parsing: none of them occurs in the translator's source, bar the words of GLSL itself and of the prelude."""
    with open(refshader.REPORT_PATH, encoding="utf-8") as f:
        rewritten = [line[6:] for line in f if line.startswith("    + ") and line.strip() != "+ (dropped)"]
    with open(os.path.join(ORACLE_DIR, "glsl_cpu.hpp"), encoding="utf-8") as f:
        prelude = set(re.findall(r"[A-Za-z_]\w*", f.read()))
    with open(os.path.join(ORACLE_DIR, "ref_translate.py"), encoding="utf-8") as f:
        translator = set(re.findall(r"[A-Za-z_]\w*", f.read()))
    names = set(re.findall(r"[A-Za-z_]\w*", " ".join(rewritten))) - prelude - {"include", "inc", "glsl", "explicit", "p"}
    assert len(names) > 20 and any(n.startswith("main_") for n in names)
    assert not names & translator, sorted(names & translator)


GOOD_GLSL = """#pragma shader_stage(compute)
#extension GL_EXT_scalar_block_layout : require
#define TWO 2
layout(local_size_x = 8, local_size_y = 8) in;
layout(buffer_reference, scalar) buffer Items { float item[]; };
layout(push_constant) uniform Push {
    Items items;   // a comment with inout and layout in it
    int count;
};
layout(binding = 0, rgba32f) restrict writeonly uniform image2D target;
/* a block comment
   with uniform in it */
void bump(inout float a, float b) { a += b * TWO; }
void main() { }
"""
BAD_GLSL = ["#version 450", "layout(std430, binding = 1) buffer B { float v[]; };", "layout(location = 0) in vec3 p;",
            "void g(out float a) { a = 1.0; }", "shared float tile[64];", "layout(binding = 0) uniform U { float x; };",
            "layout(buffer_reference, scalar) buffer Two { float a[]; float b[]; };", "#line 7", "precision highp float;"]


def test_translator_rewrites_only_what_it_recognises(tmp_path):
    """The translator on GLSL written for this test: the seven rewrites, every other line kept as it is and at its line
    number, output under OUT/gen only, and a stop with an error on any layout, qualifier or preprocessor line outside them."""
    import ref_translate
    src, out = tmp_path / "src", tmp_path / "out"
    src.mkdir()
    (src / "good.comp").write_text(GOOD_GLSL, encoding="utf-8")
    report = []
    ref_translate.translate_file(str(src), "good.comp", str(out), report, set())
    assert sorted(os.listdir(out)) == ["gen"] and os.listdir(out / "gen") == ["good.comp.inc"]
    got = (out / "gen" / "good.comp.inc").read_text(encoding="utf-8").split("\n")
    want = GOOD_GLSL.split("\n")
    assert len(got) == len(want) and len(report) == 8
    assert got[0] == got[1] == got[3] == "" and got[2] == want[2]
    assert got[4] == "struct Items { float* item; };" and got[5] == "Items items; int count;" and got[6:9] == ["", "", ""]
    assert got[9] == "image2D target;" and got[10:12] == want[10:12]
    assert got[12] == "void bump(float& a, float b) { a += b * TWO; }" and got[13] == "void main_good() { }"
    for k, line in enumerate(BAD_GLSL):
        (src / f"bad{k}.comp").write_text("float ok;\n" + line + "\n", encoding="utf-8")
        with pytest.raises(ref_translate.TranslateError, match=f"bad{k}.comp:2"):
            ref_translate.translate_file(str(src), f"bad{k}.comp", str(out), [], set())
        assert not os.path.exists(out / "gen" / f"bad{k}.comp.inc")


def test_stack_guard_drops_exactly_the_listed_cases(ref):
    """The guard, from the oracle's counters alone: what it drops is ref_cases.DROPPED, no more and no less."""
    dropped = [k for k in ref_cases.ALL if not refshader.fits_reference_stack(ref_cases.oracle_result(k)[1])]
    assert dropped == ref_cases.DROPPED
    assert ref_cases.oracle_result("atrium")[1]["ref_stack_max"] > 16        # a deep tree that does fit is among the kept


@pytest.mark.parametrize("case_id", ref_cases.KEPT)
def test_oracle_matches_reference_shader(ref, case_id):
    want = ref_cases.reference_result(ref, case_id)
    got, cnt = ref_cases.oracle_result(case_id)
    case = ref_cases.ALL[case_id]
    assert cnt["pixels"] == want.shape[0] * want.shape[1] == (case.rows or case.H) * case.W
    ref_cases.assert_same_bits(got, want, case_id)
    if case.spp == 0:
        assert np.isnan(want[..., :3]).all() and (want[..., 3] == 1.0).all()      # :312 divides by zero
    if case_id == "nan_slab":
        assert cnt["triangle_tests"] == 0 and cnt["node_pops"] == cnt["segments"]    # the NaN slab culls the root


def test_cases_reach_what_they_claim():
    """By the oracle's counters: two draw commands are both fetched, the empty scene hits nothing, 0 bounces is one segment
    a pixel and 12 bounces many, 0 samples none, some random scene tests spheres and triangles, and the random scenes hold
    both material types."""
    cnt = {k: ref_cases.oracle_result(k)[1] for k in ref_cases.KEPT}
    assert cnt["edge_two_draws_b3_s1"]["draw_fetches"] == 2 * cnt["edge_two_draws_b3_s1"]["segments"]
    assert cnt["edge_empty_b3_s1"]["hits"] == 0 and cnt["edge_no_meshes_b3_s1"]["node_pops"] == 0
    assert cnt["edge_base_b0_s1"]["segments"] == cnt["edge_base_b0_s1"]["pixels"]
    assert cnt["edge_base_b12_s1"]["segments"] > 5 * cnt["edge_base_b12_s1"]["pixels"]
    assert cnt["edge_base_b3_s0"]["segments"] == 0
    assert any(cnt[f"random{s}"]["triangle_tests"] > 0 and cnt[f"random{s}"]["sphere_tests"] > 0 for s in range(12))
    types = np.concatenate([ref_cases.scene_of(f"random{s}").materials["type"] for s in range(12)])
    assert (types == 0).any() and (types == 1).any()


@pytest.mark.parametrize("key", sorted(golden_cases.CASES))
def test_reference_shader_reproduces_the_golden_images(ref, key):
    """tests/golden/images.npz (renders of the oracle, the fixtures the GPU tests load) from the shader itself."""
    name, W, H, bounces, spp, frames = golden_cases.CASES[key]
    golden = np.load(os.path.join(os.path.dirname(__file__), "golden", "images.npz"))[key]
    s = ref_cases.get_scene(name)
    _, cnt = oracle.render_scene(s, W, H, max_bounce=bounces, samples=spp, frame=frames[0], threads=8)
    assert refshader.fits_reference_stack(cnt), (key, cnt)
    acc = None
    for n in frames:
        acc = ref.render_scene(s, W, H, max_bounce=bounces, samples=spp, frame=n, image=acc)
    ref_cases.assert_same_bits(np.ascontiguousarray(acc[..., :3]), np.ascontiguousarray(golden, dtype=np.float32), key)


# ---- sensitivity: a comparison that cannot fail proves nothing -------------------------------------------------------
# One built-in of the prelude changed per variant, as text; the variant is built into a temporary directory.
VARIANTS = {
    "mix_lerp": [("inline float mix(float x, float y, float a) { return x * (1.0f - a) + y * a; }",
                  "inline float mix(float x, float y, float a) { return x + a * (y - x); }")],
    "minmax_nan": [("inline float min(float x, float y) { return x != x ? y : (y != y ? x : (y < x ? y : x)); }",
                    "inline float min(float x, float y) { return x != x ? x : (y != y ? y : (y < x ? y : x)); }"),
                   ("inline float max(float x, float y) { return x != x ? y : (y != y ? x : (x < y ? y : x)); }",
                    "inline float max(float x, float y) { return x != x ? x : (y != y ? y : (x < y ? y : x)); }")],
    "true_division": [("{ const float s = rcp_scalar(s_); return MAP(V, GLSL_E_MUL_VS); }", "{ return a / V(s_); }")],
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_a_changed_builtin_changes_pixels(ref, variant, tmp_path):
    """mix as x + a*(y-x), min / max returning the NaN operand, vector / scalar as true division: each changes at least
    one pixel of the case set, so the comparisons above would have caught it."""
    if not refshader.reference_present():
        pytest.skip("the variants are built from the reference checkout, which is not here")
    with open(os.path.join(ORACLE_DIR, "glsl_cpu.hpp"), encoding="utf-8") as f:
        text = f.read()
    for old, new in VARIANTS[variant]:
        assert text.count(old) == 1, old
        text = text.replace(old, new)
    (tmp_path / "glsl_cpu.hpp").write_text(text, encoding="utf-8")
    shutil.copy(os.path.join(ORACLE_DIR, "ref_driver.cpp"), tmp_path / "ref_driver.cpp")
    out = tmp_path / "out"
    subprocess.run(["make", "-s", "ref", f"REFERENCE={refshader.reference_dir()}", f"REF_SRC={tmp_path}", f"REF_OUT={out}"],
                   cwd=ORACLE_DIR, check=True)
    changed = refshader.RefShader(refshader.load(str(out / "libwcpt_ref.so")))
    differing = {}
    for case_id in ref_cases.KEPT:
        c = ref_cases.ALL[case_id]
        want = ref_cases.reference_result(ref, case_id)
        got = changed.render_scene(ref_cases.scene_of(case_id), c.W, c.H, max_bounce=c.bounces, samples=c.spp, frame=c.frame,
                                   y0=c.y0, rows=c.rows, image=ref_cases.init_image(c))
        nan = np.isnan(want) & np.isnan(got)
        n = int(((got.view(np.uint32) != want.view(np.uint32)) & ~nan).any(axis=2).sum())
        if n:
            differing[case_id] = n
    print(f"{variant}: differing pixels per case {differing}")
    assert differing, f"{variant} changes no pixel of any case"
    if variant == "minmax_nan":
        assert "nan_slab" in differing        # the crafted case is the one that reaches the choice
