"""The GEMM family's dispatch rules (the header of csrc/gemm_plan.hip, include/rlt_hip.h) restated in Python, independently of
csrc/gemm_plan.hip: tests/test_gemm_plan.py compares rlt_gemm_plan - return code and every field of the record - with plan() below.

The rules are written as a case analysis on (mode, shape, operands, epilogue), with the K slabs as an explicit list of lengths, not
as the C++'s sequence of predicates.  A call is a dict: ta, tb, M, N, K, lda, ldb, ldc, flags, present / misaligned (names of
rlt_hip.native.GEMM_PTRS), drop, ws_bytes (None: no workspace).  Switches: the environment variables of the family, as a dict of
their string values (absent = default)."""
RELU, ACC = 1, 2
E_ARG, E_WORKSPACE = -1, -3
FIELDS = ("family", "ta", "tb", "fast", "persistent", "ns", "kchunk", "slab_xcd", "epilogue", "narrow")
NONE = dict({f: 0 for f in FIELDS}, family="none")


def cdiv(a, b):
    return -(-a // b)


def _num(sw, name, default):
    return int(sw[name]) if name in sw else default


def wanted_slabs(M, N, K, sw):
    """split-K fills the chip where the 128 x 128 output tiles alone do not: from K = 1024, below 256 tiles"""
    tiles = cdiv(M, 128) * cdiv(N, 128)
    if tiles >= 256 or K < _num(sw, "RLT_GEMM_SPLIT_KMIN", 1024):
        return 1
    want = max(_num(sw, "RLT_GEMM_SPLIT_TARGET", 1024) // tiles, 1)
    want = min(want, max(K // (512 if K >= 4096 else 256), 1), 256)       # at least 256 of K per slab, 512 from K = 4096
    return want // 8 * 8 if want >= 8 else want                            # whole groups of 8: a slab per XCD and round


def workspace_bytes(M, N, K, sw=None):
    want = wanted_slabs(M, N, K, sw or {})
    return (want * M * N + want * M) * 4 if want > 1 else 0


def plan(call, precision, sw=None):
    """-> (return code, record)"""
    sw = sw or {}
    c = call
    ta, tb, M, N, K, flags = int(bool(c["ta"])), int(bool(c["tb"])), c["M"], c["N"], c["K"], c["flags"]
    has = lambda n: n in c["present"]
    aligned = lambda n: n not in c["misaligned"]
    if min(M, N, K) <= 0 or c["lda"] < (M if ta else K) or c["ldb"] < (K if tb else N) or c["ldc"] < N or (has("colsum") and not ta):
        return E_ARG, NONE
    forced = sw.get("RLT_GEMM_MODE")
    mode = precision if forced is None else "bf16x6" if forced in ("bf16x6", "2") else "bf16x3" if forced in ("bf16x3", "1") else "fp32"
    bits = has("bits_out") or has("bits_in")
    relu, acc = bool(flags & RELU), bool(flags & ACC)

    # ---- K slabs: none with the 1-bit masks, none without a workspace; a short workspace is refused
    want = 1 if bits else wanted_slabs(M, N, K, sw)
    if want > 1 and c["ws_bytes"] is None:
        want = 1
    elif want > 1 and c["ws_bytes"] < workspace_bytes(M, N, K, sw):
        return E_WORKSPACE, NONE
    length = cdiv(cdiv(K, want), 32) * 32                     # whole 32-wide K tiles
    ns = cdiv(K, length)
    slabs = [length] * (ns - 1) + [K - length * (ns - 1)]
    rec = dict(NONE, ta=ta, tb=tb, fast=1, ns=ns, kchunk=length, slab_xcd=int(ns > 1 and ns % 8 == 0 and "RLT_GEMM_NO_SLAB_XCD" not in sw))

    vec = c["lda"] % 4 == 0 and c["ldb"] % 4 == 0 and aligned("A") and aligned("B")       # 16-byte loads of both operands
    tiles256 = (M // 256) * (N // 256)

    def persistent(workgroups):
        return int(not ta and ns == 1 and workgroups > 0 and workgroups % 8 == 0 and tiles256 > workgroups)

    def small(family):
        """the 128 x 128 kernels: branch-free loaders where every 16-byte load is whole and aligned"""
        fast = (vec and K % 4 == 0 and K >= 4 and (not ta or (M % 4 == 0 and M >= 4)) and (tb or (N % 4 == 0 and N >= 4))
                and _num(sw, "RLT_GEMM_NOFAST", 0) == 0)
        return 0, dict(rec, family=family, fast=int(fast))

    if mode == "bf16x6":
        # the weights-stationary kernel: the Linear layers' shape, the epilogues it has, everything 16-byte aligned
        epilogue = 3 if has("bits_in") else 2 if has("bits_out") else 1 if relu else 0
        panels = N % 256 == 0 or (K == 128 and N % 128 == 0 and not bits)
        pointers = ["A", "B", "C"] + [n for n in ("bias", "bias2", "bits_out", "bits_in") if has(n)]
        if (_num(sw, "RLT_GEMM6S", 1) != 0 and not ta and ns == 1 and K in (128, 256) and panels and 8192 <= M and N <= 65536
                and not (has("relu_mask") or has("colsum") or c["drop"] or acc or (has("bits_out") and has("bits_in")))
                and (epilogue != 3 or not (has("bias") or has("bias2") or relu))
                and all(aligned(n) for n in pointers) and c["lda"] % 4 == c["ldb"] % 4 == c["ldc"] % 4 == 0
                and c["lda"] * 128 < 2 ** 31 and c["ldc"] * 128 < 2 ** 31):
            if has("bits_out") and not relu:
                return -1, NONE
            return 0, dict(rec, family="gemm6s", ta=0, kchunk=K, epilogue=epilogue, narrow=int(N % 256 != 0))
        if not (vec and M % 256 == 0 and N % 128 == 0 and K % 32 == 0):
            return small("gemm")                              # off the six-product tiles: exact fp32
        if N % 256 or "RLT_GEMM6_SMALL" in sw:
            return 0, dict(rec, family="gemm6")
        if min(slabs) < 64 or _num(sw, "RLT_GEMM6C", 1) == 0:   # a slab of ONE K tile: no k-step pipeline
            return 0, dict(rec, family="gemm6b")
        plain = not (has("relu_mask") or bits or c["drop"])
        six_e = _num(sw, "RLT_GEMM6E", 1) != 0 and plain and (ta or K >= 1024 or _num(sw, "RLT_GEMM6E_ALL", 0) != 0)
        return 0, dict(rec, family="gemm6e" if six_e else "gemm6c", persistent=persistent(_num(sw, "RLT_GEMM6_PERSIST", 256)))
    if mode == "bf16x3":
        if vec and M % 256 == 0 and N % 256 == 0 and K % 32 == 0 and _num(sw, "RLT_GEMM_NO_BIG", 0) == 0:
            stream_b = tb or (_num(sw, "RLT_GEMM_PERSIST_NN", 0) != 0 and not has("bits_in"))
            return 0, dict(rec, family="gemm3b", persistent=int(stream_b and K >= 64 and persistent(_num(sw, "RLT_GEMM_PERSIST", 256))))
        return small("gemm3")
    return small("gemm")
