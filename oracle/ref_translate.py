"""Mechanical translation of GLSL compute shaders into text that a C++20 compiler accepts behind oracle/glsl_cpu.hpp.
TEST INFRASTRUCTURE ONLY.

    python ref_translate.py SHADER_DIR OUT_DIR FILE...

Each FILE (relative to SHADER_DIR), and every file it includes, is written under OUT_DIR/gen/ at the same relative path,
with `.inc` appended, and OUT_DIR/translate_report.txt lists every line that was rewritten. Nothing is written anywhere
else. Only these rewrites are applied, each to whole declarations or single tokens:

  * `#pragma shader_stage(...)`, `#extension ...` and `layout(local_size...) in;` are dropped;
  * `#include "p"` becomes `#include "p.inc"` (and p is translated too);
  * `layout(buffer_reference, ...) buffer N { T f[]; };` becomes `struct N { T* f; };` -- a struct holding a pointer; a member
    that is no array becomes a reference that glsl::bind_block points at the buffer;
  * `layout(push_constant) uniform N { members };` becomes the members as globals;
  * `layout(binding = ...) [qualifiers] uniform T name;` becomes the global `T name;`;
  * a parameter `inout T x` becomes `T& x`;
  * `void main()` becomes `void main_<file stem>()`.

Every identifier comes from the declarations parsed; no name of any shader is written here. Any other `layout`, storage or
parameter qualifier, or preprocessor line stops the translation with an error. Float constants stay as written: the
compile flag -fsingle-precision-constant makes them binary32.
"""
import os
import re
import sys

PREPROCESSOR_KEPT = ("define", "ifndef", "ifdef", "if", "else", "elif", "endif", "undef")
# GLSL qualifiers that must not survive into the output (const is C++'s too and stays)
QUALIFIERS = {"inout", "out", "in", "uniform", "buffer", "restrict", "writeonly", "readonly", "coherent", "volatile",
              "shared", "flat", "smooth", "noperspective", "varying", "attribute", "highp", "mediump", "lowp", "precision",
              "invariant", "centroid", "patch", "sample", "subroutine", "layout", "precise"}
IMAGE_QUALIFIERS = {"restrict", "writeonly", "readonly", "coherent", "volatile"}
IDENT = r"[A-Za-z_][A-Za-z_0-9]*"


class TranslateError(Exception):
    pass


def strip_comments(line, in_block):
    """The code of one line with comments blanked out, and whether a block comment is still open after it."""
    out, i = [], 0
    while i < len(line):
        if in_block:
            j = line.find("*/", i)
            if j < 0:
                return "".join(out), True
            i, in_block = j + 2, False
        elif line.startswith("//", i):
            break
        elif line.startswith("/*", i):
            in_block, i = True, i + 2
        else:
            out.append(line[i])
            i += 1
    return "".join(out), in_block


def _members(body, where):
    """[(type, name, is_array)] of the member declarations `T name;` / `T name[];` in a block's body."""
    found = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.fullmatch(rf"({IDENT})\s+({IDENT})\s*(\[\s*\])?", decl)
        if not m:
            raise TranslateError(f"{where}: member declaration not understood: {decl!r}")
        found.append((m.group(1), m.group(2), m.group(3) is not None))
    return found


def _layout(code, where):
    """The replacement text of one complete `layout...;` declaration (comments already removed)."""
    m = re.fullmatch(r"layout\s*\(([^)]*)\)\s*(.*)", code.strip(), re.S)
    if not m:
        raise TranslateError(f"{where}: layout declaration not understood: {code!r}")
    args = [a.strip() for a in m.group(1).split(",")]
    rest = m.group(2).strip()
    keys = [a.split("=")[0].strip() for a in args]
    if all(k in ("local_size_x", "local_size_y", "local_size_z") for k in keys) and rest == "in;":
        return ""
    if "buffer_reference" in keys and set(keys) <= {"buffer_reference", "scalar"}:
        b = re.fullmatch(rf"buffer\s+({IDENT})\s*\{{(.*)\}}\s*;", rest, re.S)
        if not b:
            raise TranslateError(f"{where}: buffer_reference block not understood: {rest!r}")
        members = _members(b.group(2), where)
        if len(members) != 1:
            raise TranslateError(f"{where}: a buffer_reference block with {len(members)} members")
        (mtype, mname, is_array), = members
        name = b.group(1)
        if is_array:
            return f"struct {name} {{ {mtype}* {mname}; }};"
        return (f"struct {name} {{ {mtype}& {mname}; {name}() : {mname}(glsl::unbound_block<{mtype}>()) {{}} "
                f"explicit {name}({mtype}* p) : {mname}(*p) {{}} }};")
    if keys == ["push_constant"]:
        b = re.fullmatch(rf"uniform\s+{IDENT}\s*\{{(.*)\}}\s*;", rest, re.S)
        if not b:
            raise TranslateError(f"{where}: push_constant block not understood: {rest!r}")
        members = _members(b.group(1), where)
        if any(is_array for _, _, is_array in members):
            raise TranslateError(f"{where}: an array in a push_constant block")
        return " ".join(f"{t} {n};" for t, n, _ in members)
    if keys[0] == "binding" and all(re.fullmatch(r"(rgba|rg|r)(8|16|32)(f|i|ui|_snorm)?", k) for k in keys[1:]):
        words = rest.rstrip(";").split()
        if not rest.endswith(";") or len(words) < 3 or words[-3] != "uniform" or not set(words[:-3]) <= IMAGE_QUALIFIERS:
            raise TranslateError(f"{where}: binding declaration not understood: {rest!r}")
        if not all(re.fullmatch(IDENT, w) for w in words[-2:]):
            raise TranslateError(f"{where}: binding declaration not understood: {rest!r}")
        return f"{words[-2]} {words[-1]};"
    raise TranslateError(f"{where}: layout({m.group(1)}) not recognised")


def translate_file(shader_dir, rel, out_dir, report, done):
    if rel in done:
        return
    done.add(rel)
    src = os.path.join(shader_dir, rel)
    stem = re.sub(r"\W", "_", os.path.splitext(os.path.basename(rel))[0])
    with open(src, encoding="utf-8") as f:
        lines = f.read().split("\n")
    out, in_block, pending, pending_at = [], False, None, 0

    def emit(n, old, new, what):
        report.append(f"{rel}:{n}: {what}\n    - {old.strip()}\n    + {new.strip() or '(dropped)'}")
        out.append(new)

    for n, line in enumerate(lines, 1):
        where = f"{rel}:{n}"
        code, in_block = strip_comments(line, in_block)
        if pending is not None:                       # inside a layout declaration that spans lines
            pending += " " + code
            if code.rstrip().endswith(";") and pending.count("{") == pending.count("}"):
                emit(pending_at, pending, _layout(pending, f"{rel}:{pending_at}"), "layout declaration")
                out.extend([""] * (n - pending_at))     # keep the line numbers
                pending = None
            continue
        s = code.strip()
        if s.startswith("#"):
            m = re.match(r"#\s*(\w+)\s*(.*)", s)
            directive, arg = (m.group(1), m.group(2)) if m else ("", "")
            if directive == "pragma" and arg.startswith("shader_stage"):
                emit(n, line, "", "pragma dropped")
            elif directive == "extension":
                emit(n, line, "", "extension dropped")
            elif directive == "include":
                inc = re.fullmatch(r'"([^"]+)"', arg.strip())
                if not inc:
                    raise TranslateError(f"{where}: include not understood: {s!r}")
                translate_file(shader_dir, os.path.normpath(os.path.join(os.path.dirname(rel), inc.group(1))), out_dir,
                               report, done)
                emit(n, line, f'#include "{inc.group(1)}.inc"', "include")
            elif directive in PREPROCESSOR_KEPT:
                out.append(line)
            else:
                raise TranslateError(f"{where}: preprocessor line not recognised: {s!r}")
            continue
        if re.match(r"layout\b", s):
            if s.endswith(";") and s.count("{") == s.count("}"):
                emit(n, line, _layout(s, where), "layout declaration")
            else:
                pending, pending_at = s, n
            continue
        new = line
        if code.strip():
            new_code = re.sub(rf"\binout\s+({IDENT})\s+({IDENT})", r"\1& \2", code)
            new_code = re.sub(r"\bvoid\s+main\s*\(\s*\)", f"void main_{stem}()", new_code)
            left = QUALIFIERS & set(re.findall(IDENT, new_code))
            if left:
                raise TranslateError(f"{where}: qualifier not recognised here: {sorted(left)} in {s!r}")
            if new_code != code:
                new = line.replace(code, new_code, 1) if code in line else new_code
                emit(n, line, new, "main renamed" if "main_" in new_code and "main_" not in code else "inout parameter")
                continue
        out.append(new)
    if pending is not None or in_block:
        raise TranslateError(f"{rel}: ends inside a declaration or a comment")
    dst = os.path.join(out_dir, "gen", rel + ".inc")
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    with open(dst, "w", encoding="utf-8") as f:
        f.write("\n".join(out))


def main(argv):
    if len(argv) < 4:
        sys.exit(__doc__)
    shader_dir, out_dir, files = argv[1], argv[2], argv[3:]
    report, done = [], set()
    try:
        for rel in files:
            translate_file(shader_dir, rel, out_dir, report, done)
    except TranslateError as e:
        sys.exit(f"ref_translate: {e}")
    with open(os.path.join(out_dir, "translate_report.txt"), "w", encoding="utf-8") as f:
        f.write(f"{len(done)} files translated, {len(report)} lines rewritten\n" + "\n".join(report) + "\n")


if __name__ == "__main__":
    main(sys.argv)
