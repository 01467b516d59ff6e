"""Things csrc/ must not grow back (no compilation, no GPU):

  * compile-time A/B switches that nothing builds: every macro a preprocessor conditional under csrc/ tests is on a list written
    here - the builds a committed tool or test asks for, and nothing else;
  * private copies of the bf16 split primitives: no .hip file defines a function that csrc/split6.h defines;
  * private copies of what the GEMM family files share: gemm_common.h, gemm3.h, gemm6c.h.
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


def test_no_private_copy_of_the_gemm_frame():
    """what the GEMM family files share is defined once: in gemm_common.h, or in the header of the family that introduced it"""
    texts = dict(_sources())
    shared = {h: _defined_functions(texts[h]) for h in ("gemm_common.h", "gemm3.h", "gemm6c.h")}
    assert {"xcd_remap", "decode_block", "tile_frame", "next_tile", "gemm_epilogue", "write_output_t", "write_output", "write_output_simple", "accumulate_blocks",
            "csum_add", "finish_colsum", "family_is"} <= shared["gemm_common.h"], sorted(shared["gemm_common.h"])
    assert {"prow2", "swz2", "kcb_row", "load3b"} <= shared["gemm3.h"] and {"phys6"} <= shared["gemm6c.h"]
    for header, names in shared.items():
        clashes = {name: sorted(_defined_functions(text) & names) for name, text in texts.items() if name != header}
        clashes = {k: v for k, v in clashes.items() if v}
        assert not clashes, f"defined in csrc/{header} and again in: {clashes}"
    # and the constants two files need
    for const, header in (("BK3", "gemm3.h"), ("BM2", "gemm3.h"), ("PL2", "gemm3.h"), ("HB6", "gemm6c.h"), ("KB6", "gemm6c.h")):
        holders = [name for name, text in texts.items() if re.search(r"constexpr\s+int\s+[^;]*\b%s\s*=" % const, text)]
        assert holders == [header], (const, holders)
