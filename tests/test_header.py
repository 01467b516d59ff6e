"""rlt_hip/header.py, which derives the ctypes binding from include/rlt_hip.h: its rules on literal snippets, then the hand-written
ctypes.Structure mirrors and the integer constants of rlt_hip/native.py against what it reads from the real header.  No device."""
from ctypes import c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint32, c_void_p as P

import pytest

from rlt_hip import header, native


def test_pointers_of_any_kind_are_void_pointers():
    text = "int rlt_f(const float* const* x, float* const* y, const rlt_thing* t, struct rlt_tag* u, void* s, const void *w, int n[4]);"
    assert header.parse(text)[1] == {"rlt_f": (c_int, [P] * 7)}


def test_scalars_void_list_and_char_pointer_return():
    sig = header.parse("size_t rlt_a(size_t n, int m);\ndouble rlt_b(double x, float y);\nint rlt_c(uint32_t seed, int64_t t, int32_t k);\n"
                       "int rlt_version(void);\nconst char* rlt_name(int code);\nsize_t rlt_bytes( void );")[1]
    assert sig["rlt_a"] == (c_size_t, [c_size_t, c_int]) and c_size_t is not c_int
    assert sig["rlt_b"] == (c_double, [c_double, c_float]) and c_double is not c_float
    assert sig["rlt_c"] == (c_int, [c_uint32, c_int64, c_int32]) and c_int64 is not c_int32
    assert (sig["rlt_version"], sig["rlt_name"], sig["rlt_bytes"]) == ((c_int, []), (c_char_p, [c_int]), (c_size_t, []))
    assert list(sig) == ["rlt_a", "rlt_b", "rlt_c", "rlt_version", "rlt_name", "rlt_bytes"]


def test_prototype_over_three_lines_with_a_call_in_a_comment():
    text = """/* rlt_old(int a); is gone */
    #define RLT_LIMIT (-3)   /* rlt_macro( */
    int rlt_g(const float* p, int B,   /* as rlt_foo( takes it */
              double tau,              // and rlt_bar(
              size_t ws_bytes, void* stream);"""
    assert header.parse(text)[:2] == ({"RLT_LIMIT": -3}, {"rlt_g": (c_int, [P, c_int, c_double, c_size_t, P])})


@pytest.mark.parametrize("text, named", [
    ("int rlt_h(int n, unsigned flags);", "rlt_h"),                       # a scalar outside the map
    ("int rlt_h(long n);", "rlt_h"),
    ("int rlt_h(rlt_thing by_value);", "rlt_h"),
    ("long rlt_h(int n);", "rlt_h"),                                      # ... as the return type
    ("float* rlt_h(int n);", "rlt_h"),
    ("int rlt_h(int (*callback)(int));", "rlt_h"),                        # not a prototype of the header's style
    ("int rlt_h(int n) { return n; }", "rlt_h"),
    ("#define RLT_SCALE 1.5f", "RLT_SCALE"),
    ("typedef struct { short s; } rlt_t;", "rlt_t"),
    ("typedef struct { float g[RLT_UNKNOWN]; } rlt_t;", "rlt_t"),         # an array size that is no integer and no define
    ("int rlt_h(float g[N+1]);", "rlt_h"),
])
def test_whatever_the_reader_does_not_know_raises_and_is_named(text, named):
    with pytest.raises(RuntimeError, match=named):
        header.parse(text)


def test_struct_bodies():
    text = """#define RLT_N 8
    typedef struct { int family; float beta; float gain[RLT_N]; const float* discount; } rlt_spec;
    typedef struct rlt_w { const float *w_ih[2], *b; } rlt_w;
    struct rlt_plan { int fwd, bwd; size_t bytes; };
    int rlt_plan(int B, struct rlt_plan* out, const rlt_spec* spec);"""
    _, sig, structs = header.parse(text)
    assert structs == {"rlt_spec": [("family", c_int), ("beta", c_float), ("gain", c_float * 8), ("discount", P)],
                       "rlt_w": [("w_ih", P * 2), ("b", P)], "rlt_plan": [("fwd", c_int), ("bwd", c_int), ("bytes", c_size_t)]}
    assert sig == {"rlt_plan": (c_int, [c_int, P, P])}


def test_missing_header_is_a_runtime_error_with_the_path(tmp_path):
    with pytest.raises(RuntimeError, match="no_such_header.h"):
        header.read(str(tmp_path / "no_such_header.h"))


MIRRORS = {"rlt_encoder_weights": "EncoderPtrs", "rlt_encoder_grads": "EncoderPtrs", "rlt_lstm_layer_weights": "LstmLayerPtrs",
           "rlt_lstm_layer_grads": "LstmLayerPtrs", "rlt_sparse_batch": "SparseBatchPtrs", "rlt_recipe": "RecipeStruct",
           "rlt_reward_spec": "RewardSpecStruct", "rlt_paired_compare_plan": "PairedComparePlan", "rlt_gemm_dispatch": "GemmDispatch",
           "rlt_gemm_call": "GemmCall", "rlt_attention_plan": "AttentionPlan", "rlt_bilstm_rec_plan": "BilstmRecPlan"}


@pytest.mark.parametrize("struct", sorted(MIRRORS))
def test_structure_mirrors_equal_the_header_structs(struct):
    """Field count, order, names and ctypes."""
    assert list(getattr(native, MIRRORS[struct])._fields_) == native.STRUCTS[struct]


def test_structs_without_a_mirror_are_the_device_records():
    """The header's remaining structs are device records that Python reads as words: a new host struct needs a mirror here."""
    assert set(native.STRUCTS) - set(MIRRORS) == {"rlt_opt_state", "rlt_grad_seg", "rlt_recipe_group", "rlt_recipe_state"}


def test_constants_equal_the_header_defines():
    """Every RLT_<NAME> with a Python mirror - native.<NAME>, or the one renamed mirror - has the header's value: a number that
    someone types again in native.py and that drifts fails here."""
    renamed = {"RLT_COMPARE_MAX_SYSTEMS": "CMP_MAX_SYSTEMS"}
    mirrored = {d: renamed.get(d, d[4:]) for d in native.DEFINES if hasattr(native, renamed.get(d, d[4:]))}
    for define, name in mirrored.items():
        assert getattr(native, name) == native.DEFINES[define], (define, name)
    assert {d.split("_")[1] for d in mirrored} >= {"ABI", "METRIC", "LOSS", "GEMM", "HEAD", "PROBE", "CUT", "SWEEP", "REWARD", "PAIR", "SEQ",
                                                   "PRECISION", "OP", "SPARSE", "CMP", "COMPARE"} and len(mirrored) >= 55
    assert native.DEFINES["RLT_ABI_VERSION"] == 5 and native.DEFINES["RLT_PRECISION_DEFAULT"] == -1 and native.DEFINES["RLT_E_ALIGN"] == -4
