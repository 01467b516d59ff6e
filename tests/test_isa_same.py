"""tools/isa_same.py --by-kernel: the cut of an assembly file into one record per kernel, and the comparison of two sets of records,
on hand-written assembly.  CPU only, nothing is compiled."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(REPO, "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)

import isa_same as I  # noqa: E402


def kernel(name, n, body="\tv_add_f32_e32 v0, v1, v2", cuid="0123abcd"):
    """a kernel as hipcc writes it: the n-th function of its file"""
    return f"""\t.section\t.text.{name},"axG",@progbits,{name},comdat
\t.globl\t{name}
\t.p2align\t8
\t.type\t{name},@function
{name}: ; @{name}
.Lfunc_begin{n}:
; %bb.0:
\ts_cmp_lt_i32 s0, 1
\ts_cbranch_scc1 .LBB{n}_2
; %bb.1:                                ;   in Loop: Header=BB{n}_2 Depth=1
{body}
.LBB{n}_2:
\ts_getpc_b64 s[0:1]
\ts_add_u32 s0, s0, __hip_cuid_{cuid}@rel32@lo+4
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel {name}
\t\t.amdhsa_next_free_vgpr 3
\t.end_amdhsa_kernel
\t.section\t.text.{name},"axG",@progbits,{name},comdat
.Lfunc_end{n}:
\t.size\t{name}, .Lfunc_end{n}-{name}
\t.set {name}.num_vgpr, 3
"""


DEVICE_FUNCTION = """helper: ; @helper
\tv_mov_b32_e32 v0, 0
\ts_setpc_b64 s[30:31]
.Lfunc_end9:
"""


def test_a_record_per_kernel_and_nothing_else():
    text = "\t.text\n" + kernel("k_a", 0) + DEVICE_FUNCTION + kernel("k_b", 1) + "\t.amdgpu_metadata\n"
    recs = I.kernel_records(text)
    assert sorted(recs) == ["k_a", "k_b"]                       # `helper` has no .amdhsa_kernel block
    assert recs["k_a"].startswith("k_a: ; @k_a\n") and recs["k_a"].endswith(".Lfunc_end#:")
    assert ".amdhsa_next_free_vgpr 3" in recs["k_a"] and "v_add_f32_e32" in recs["k_a"]
    assert ".set k_a.num_vgpr" not in recs["k_a"] and "k_b" not in recs["k_a"]


def test_the_same_kernel_at_two_ordinals_in_two_directories_is_the_same():
    a = I.kernel_records(kernel("k", 3, cuid="0123abcd"))["k"]
    b = I.kernel_records(kernel("other", 0) + kernel("k", 17, cuid="fedc9876"))["k"]
    assert a == b
    assert ".LBB#_2" in a and "17" not in b and "fedc9876" not in b


def test_one_changed_instruction_is_different():
    a = I.kernel_records(kernel("k", 3))
    b = I.kernel_records(kernel("k", 3, body="\tv_sub_f32_e32 v0, v1, v2"))
    assert a["k"] != b["k"]
    assert I.compare_records([a], [b]) == [("k", "DIFFERENT", 1)]


def test_sets_are_compared_whatever_file_a_record_is_in():
    one_file = [I.kernel_records(kernel("shared", 0) + kernel("k_a", 1) + kernel("k_b", 2))]
    split = [I.kernel_records(kernel("shared", 0) + kernel("k_b", 1)), I.kernel_records(kernel("shared", 0) + kernel("k_a", 1))]
    assert I.compare_records(one_file, split) == [("k_a", "same", 1), ("k_b", "same", 1), ("shared", "same", 2)]
    # lost, added, and a copy of a shared kernel that differs from the others
    changed = [split[0], I.kernel_records(kernel("shared", 0, body="\ts_nop 0") + kernel("k_c", 1))]
    assert I.compare_records(one_file, changed) == [("k_a", "missing", 0), ("k_b", "same", 1), ("k_c", "new", 1), ("shared", "DIFFERENT", 2)]
