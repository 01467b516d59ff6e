"""Two things csrc/ must not grow back (no compilation, no GPU):

  * compile-time A/B switches that nothing builds: every macro a preprocessor conditional under csrc/ tests is on a list written
    here - the builds a committed tool or test asks for, and nothing else;
  * private copies of the bf16 split primitives: no .hip file defines a function that csrc/split6.h defines.
"""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "ranked-list-truncation_amd", "csrc")

# used by a committed tool or build: the host-only sanitizer build (rlt_hip/build.py), the stamps builds of tools/bench_kernels.py and
# tools/pp_stamps.py, the include-name overrides of the body generators' timing modes
KEPT = {"RLT_BOUNDS_CHECK", "RLT_HOST_ONLY", "RLT_STAMPS", "RLT_PP_STAMPS", "RLT_DKV1_STAMPS", "RLT_A6N_STAMPS", "RLT_A6H_STAMPS",
        "RLT_A6N_DQ1_BODY", "RLT_A6H_FWD1_BODY"}


def _sources():
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h", ".inc")):
            with open(os.path.join(CSRC, name)) as f:
                yield name, f.read()


def test_every_conditional_macro_is_accounted_for():
    seen = {}
    for name, text in _sources():
        for line in re.findall(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b(.*)$", text, flags=re.M):
            for macro in re.findall(r"\b[A-Za-z_]\w*\b", line.split("//")[0]):
                if macro != "defined":
                    seen.setdefault(macro, set()).add(name)
    extra = {m: sorted(files) for m, files in seen.items() if m not in KEPT}
    assert not extra, f"compile-time switches that no committed tool or build passes: {extra}"
    assert all(m in seen for m in KEPT), sorted(KEPT - set(seen))


def _defined_functions(text):
    # `name(` at the end of a declarator that starts a line with a type or an attribute, followed by a body on the same or a later line
    return set(re.findall(r"^(?:template\s*<[^>]*>\s*)?(?:__device__|__host__|static|inline|constexpr)[^;{()=]*?\b([A-Za-z_]\w*)\s*\([^;{]*\)\s*(?:->[^;{]*)?\{",
                          text, flags=re.M))


def test_no_private_copy_of_a_split_primitive():
    texts = dict(_sources())
    shared = _defined_functions(texts["split6.h"])
    assert {"pk2", "lo16", "hi16", "frag4", "cat2", "split4", "split8", "split4x3", "split8x3", "split8x3_by_pair", "mfma3", "mfma6", "tr_read", "cat_frag",
            "col_max4", "col_sum4", "split6_part", "x6_plane_a", "x6_plane_b"} <= shared, sorted(shared)
    clashes = {name: sorted(_defined_functions(text) & shared) for name, text in texts.items() if name.endswith(".hip")}
    clashes = {k: v for k, v in clashes.items() if v}
    assert not clashes, f"defined in csrc/split6.h and again in: {clashes}"
