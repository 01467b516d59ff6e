"""The case table of the GEMM family's dispatch: one id per (kernel family, operand layout, variant), each with the fields of the
dispatch record it is about.  tests/test_gemm_dispatch_gpu.py launches every id on the device and asserts rlt_gemm_last_dispatch
against `want`; tests/test_gemm_plan.py asserts rlt_gemm_plan against it on the CPU."""
MODES = {"fp32": 0, "bf16x3": 1, "bf16x6": 2}
LAYOUTS = {"nn": (0, 0), "nt": (0, 1), "tn": (1, 0), "tt": (1, 1)}
RELU, ACC = 1, 2

CASES = {}


def case(name, mode, layout, M, Nn, K, want, **opt):
    """want: the fields of the dispatch record this case is about (family always)."""
    ta, tb = LAYOUTS[layout]
    assert name not in CASES, name
    CASES[name] = dict(mode=mode, ta=ta, tb=tb, M=M, N=Nn, K=K, want=dict(want, ta=ta, tb=tb), **opt)


def _loader_cases(fam, mode):
    """gemm_kernel / gemm3_kernel: the branch-free loaders and every single cause that sends a shape to the guarded ones"""
    for lay, (ta, tb) in LAYOUTS.items():
        w = lambda fast: dict(family=fam, fast=int(fast), ns=1)
        case(f"{fam}-{lay}-fast-132x136x40", mode, lay, 132, 136, 40, w(True), bias=True)
        case(f"{fam}-{lay}-slow-K38", mode, lay, 132, 136, 38, w(False))
        case(f"{fam}-{lay}-slow-K3", mode, lay, 132, 136, 3, w(False), bias=True)
        case(f"{fam}-{lay}-slow-lda", mode, lay, 132, 136, 40, w(False), lda_pad=5)
        case(f"{fam}-{lay}-slow-ldb", mode, lay, 132, 136, 40, w(False), ldb_pad=5)
        case(f"{fam}-{lay}-slow-Aoff4", mode, lay, 132, 136, 40, w(False), a_off=1)
        case(f"{fam}-{lay}-slow-Boff4", mode, lay, 132, 136, 40, w(False), b_off=1, relu=True)
        # M % 4 with A stored [K][M], N % 4 with B stored [K][N]: slow there, the fast loader's ragged tile elsewhere
        case(f"{fam}-{lay}-{'slow' if ta else 'fast'}-M129", mode, lay, 129, 136, 40, w(not ta), bias=True, bias2=True)
        case(f"{fam}-{lay}-{'fast' if tb else 'slow'}-N130", mode, lay, 132, 130, 40, w(tb), acc=True)
        case(f"{fam}-{lay}-{'fast' if tb else 'slow'}-N3", mode, lay, 132, 3, 40, w(tb), bias=True)
        case(f"{fam}-{lay}-{'slow' if ta else 'fast'}-M5", mode, lay, 5, 136, 40, w(not ta))
        case(f"{fam}-{lay}-{'fast' if tb and not ta else 'slow'}-129x130x64", mode, lay, 129, 130, 64, w(tb and not ta), bias=True, relu=True, acc=True)


_loader_cases("gemm", "fp32")
_loader_cases("gemm3", "bf16x3")
case("gemm-tn-fast-mask-colsum-300x200x76", "fp32", "tn", 300, 200, 76, dict(family="gemm", fast=1), mask=True, colsum=True)
case("gemm-nt-bits-out-300x96x40", "fp32", "nt", 300, 96, 40, dict(family="gemm", fast=1), bias=True, relu=True, bits="out")
case("gemm-nn-bits-in-300x96x40", "fp32", "nn", 300, 96, 40, dict(family="gemm", fast=1), bits="in")
case("gemm-nt-drop-300x96x40", "fp32", "nt", 300, 96, 40, dict(family="gemm", fast=1), bias=True, relu=True, drop=True)
case("gemm3-tn-slow-mask-colsum-301x200x77", "bf16x3", "tn", 301, 200, 77, dict(family="gemm3", fast=0), mask=True, colsum=True)

for lay, (ta, tb) in LAYOUTS.items():
    # gemm3b: 256 x 256 tiles of the bf16x3 mode
    case(f"gemm3b-{lay}-plain-256x512x96", "bf16x3", lay, 256, 512, 96, dict(family="gemm3b", persistent=0, ns=1), bias=True, colsum=bool(ta))
    case(f"gemm3b-{lay}-split4-256x256x1024", "bf16x3", lay, 256, 256, 1024, dict(family="gemm3b", persistent=0, ns=4, kchunk=256, slab_xcd=0),
         bias=True, bias2=True, relu=True, acc=True, colsum=bool(ta))
    # gemm6: 256 x 128 tiles (N % 256 != 0)
    case(f"gemm6-{lay}-256x384x64", "bf16x6", lay, 256, 384, 64, dict(family="gemm6", ns=1), bias=True, colsum=bool(ta))
    # gemm6b: a K slab of ONE 32-wide tile
    case(f"gemm6b-{lay}-K32-256x256x32", "bf16x6", lay, 256, 256, 32, dict(family="gemm6b", ns=1, kchunk=32), bias=True, colsum=bool(ta))
    # gemm6c: the epilogues gemm6e does not have keep every layout here; without one, A stored [M][K] below K = 1024
    case(f"gemm6c-{lay}-mask-256x512x96", "bf16x6", lay, 256, 512, 96, dict(family="gemm6c", persistent=0, ns=1), mask=True, bias=True, colsum=bool(ta))
    case(f"gemm6c-{lay}-drop-256x256x96", "bf16x6", lay, 256, 256, 96, dict(family="gemm6c", persistent=0, ns=1), drop=True, bias=True, relu=True)
    case(f"gemm6c-{lay}-bits-out-256x256x96", "bf16x6", lay, 256, 256, 96, dict(family="gemm6c", persistent=0, ns=1), bits="out", bias=True, relu=True)
    case(f"gemm6c-{lay}-bits-out-drop-256x256x64", "bf16x6", lay, 256, 256, 64, dict(family="gemm6c", persistent=0, ns=1), bits="out", bias=True, relu=True, drop=True)
    case(f"gemm6c-{lay}-bits-in-512x256x96", "bf16x6", lay, 512, 256, 96, dict(family="gemm6c", persistent=0, ns=1), bits="in")
    case(f"gemm6c-{lay}-split4-mask-256x256x1024", "bf16x6", lay, 256, 256, 1024, dict(family="gemm6c", persistent=0, ns=4, kchunk=256, slab_xcd=0),
         mask=True, bias=True, acc=True, colsum=bool(ta))
    # gemm6e: A stored [K][M] at any K, A stored [M][K] from K = 1024; split-K with and without XCD-pinned slabs
    case(f"gemm6e-{lay}-split4-256x256x1024", "bf16x6", lay, 256, 256, 1024, dict(family="gemm6e", persistent=0, ns=4, kchunk=256, slab_xcd=0),
         bias=True, colsum=bool(ta))
    case(f"gemm6e-{lay}-split5-256x256x1280", "bf16x6", lay, 256, 256, 1280, dict(family="gemm6e", persistent=0, ns=5, kchunk=256, slab_xcd=0),
         bias=True, bias2=True, relu=True, acc=True, colsum=bool(ta))
    case(f"gemm6e-{lay}-split8-xcd-256x256x2048", "bf16x6", lay, 256, 256, 2048, dict(family="gemm6e", persistent=0, ns=8, kchunk=256, slab_xcd=1),
         relu=True, colsum=bool(ta))
    case(f"gemm6e-{lay}-short-last-slab-256x256x1184", "bf16x6", lay, 256, 256, 1184, dict(family="gemm6e", persistent=0, ns=4, kchunk=320, slab_xcd=0),
         acc=True, colsum=bool(ta))
    case(f"gemm6e-{lay}-unsplit-2048x2048x1024", "bf16x6", lay, 2048, 2048, 1024, dict(family="gemm6e", persistent=0, ns=1), bias=True)

for lay in ("nn", "nt"):
    case(f"gemm6c-{lay}-plain-256x256x96", "bf16x6", lay, 256, 256, 96, dict(family="gemm6c", persistent=0, ns=1), bias=True, relu=True, acc=True)
    # persistent forms: 17 x 16 tiles of 256 x 256 over 256 workgroups - 16 of them take a second tile
    case(f"gemm6c-{lay}-persistent-4352x4096x64", "bf16x6", lay, 4352, 4096, 64, dict(family="gemm6c", persistent=1, ns=1), bias=True)
    case(f"gemm6e-{lay}-persistent-4352x4096x1024", "bf16x6", lay, 4352, 4096, 1024, dict(family="gemm6e", persistent=1, ns=1), bias=True, relu=True)
for lay in ("tn", "tt"):
    case(f"gemm6e-{lay}-plain-256x256x96", "bf16x6", lay, 256, 256, 96, dict(family="gemm6e", persistent=0, ns=1), bias=True, relu=True, acc=True, colsum=True)
    case(f"gemm6e-{lay}-more-tiles-than-wgs-4352x4096x64", "bf16x6", lay, 4352, 4096, 64, dict(family="gemm6e", persistent=0, ns=1), colsum=True)
    # 24 slabs of 544, the last one a single K tile of 32: split-K on gemm6b, slabs pinned to XCDs
    case(f"gemm6b-{lay}-split24-last-slab-one-tile-256x256x12544", "bf16x6", lay, 256, 256, 12544,
         dict(family="gemm6b", ns=24, kchunk=544, slab_xcd=1), bias=True, colsum=True)
case("gemm6-tn-split4-256x128x1024", "bf16x6", "tn", 256, 128, 1024, dict(family="gemm6", ns=4, kchunk=256), bias=True, colsum=True)
case("gemm3b-nt-persistent-4352x4096x64", "bf16x3", "nt", 4352, 4096, 64, dict(family="gemm3b", persistent=1, ns=1), bias=True, relu=True)
case("gemm3b-nn-more-tiles-than-wgs-4352x4096x64", "bf16x3", "nn", 4352, 4096, 64, dict(family="gemm3b", persistent=0, ns=1), bias=True)
case("gemm3b-tn-more-tiles-than-wgs-4352x4096x64", "bf16x3", "tn", 4352, 4096, 64, dict(family="gemm3b", persistent=0, ns=1), colsum=True)
# an operand off 16 bytes on a shape of the 256 x 256 tiles: the guarded loaders of the 128 x 128 kernels
case("gemm-nt-x6-Aoff4-256x256x96", "bf16x6", "nt", 256, 256, 96, dict(family="gemm", fast=0), a_off=1, bias=True)
case("gemm-tn-x6-Boff4-256x256x96", "bf16x6", "tn", 256, 256, 96, dict(family="gemm", fast=0), b_off=1, colsum=True)
case("gemm3-nt-Boff4-256x256x96", "bf16x3", "nt", 256, 256, 96, dict(family="gemm3", fast=0), b_off=1, bias=True)

# gemm6s: the weights-stationary kernel, every instantiation: K 256 / 128 x epilogue 0-3 x both weight layouts on 256-column panels,
# K 128 x epilogue 0 / 1 x both layouts on 128-column panels.  8192 + 31 rows, one panel: 257 blocks of 32 rows over 256 streams
for lay in ("nn", "nt"):
    for K in (256, 128):
        for epi, opt in enumerate((dict(bias=True), dict(bias=True, bias2=True, relu=True), dict(bias=True, relu=True, bits="out"), dict(bits="in"))):
            case(f"gemm6s-{lay}-K{K}-wide-epi{epi}-8223x256", "bf16x6", lay, 8223, 256, K, dict(family="gemm6s", epilogue=epi, narrow=0, ns=1), **opt)
    for epi, opt in enumerate((dict(bias=True, bias2=True), dict(bias=True, relu=True))):
        case(f"gemm6s-{lay}-K128-narrow-epi{epi}-8223x384", "bf16x6", lay, 8223, 384, 128, dict(family="gemm6s", epilogue=epi, narrow=1, ns=1), **opt)
case("gemm6s-nt-K256-wide-epi0-several-blocks-per-stream-8223x2048", "bf16x6", "nt", 8223, 2048, 256, dict(family="gemm6s", epilogue=0, narrow=0), bias=True)
case("gemm-nt-x6-one-row-short-of-gemm6s-8191x256x256", "bf16x6", "nt", 8191, 256, 256, dict(family="gemm", fast=1), bias=True)
case("gemm6c-nt-one-tile-short-of-gemm6s-7936x256x256", "bf16x6", "nt", 7936, 256, 256, dict(family="gemm6c", persistent=0), bias=True)
case("gemm6c-nt-misaligned-bias-off-gemm6s-8448x256x256", "bf16x6", "nt", 8448, 256, 256, dict(family="gemm6c", persistent=0), bias=True, bias_off=1)

# split-K and its reduce in every mode: z tail of the float4 reduce (ns = 5), XCD-pinned slabs (ns = 8), a short last slab, a slab
# count changed by rounding the slab length to 32, the scalar reduce (N % 4 != 0), column sums through the slabs, the whole epilogue
# applied once in the reduce
for mode, fam in (("fp32", "gemm"), ("bf16x3", "gemm3")):
    for lay, (ta, tb) in LAYOUTS.items():
        case(f"{fam}-{lay}-split4-128x128x1024", mode, lay, 128, 128, 1024, dict(family=fam, ns=4, kchunk=256, slab_xcd=0), bias=True, colsum=bool(ta))
        case(f"{fam}-{lay}-split5-128x128x1280", mode, lay, 128, 128, 1280, dict(family=fam, ns=5, kchunk=256, slab_xcd=0),
             bias=True, bias2=True, relu=True, acc=True, colsum=bool(ta))
        case(f"{fam}-{lay}-split8-xcd-128x128x2048", mode, lay, 128, 128, 2048, dict(family=fam, ns=8, kchunk=256, slab_xcd=1), relu=True, colsum=bool(ta))
        case(f"{fam}-{lay}-split4-short-last-slab-128x128x1030", mode, lay, 128, 128, 1030, dict(family=fam, ns=4, kchunk=288, slab_xcd=0, fast=0),
             bias=True, colsum=bool(ta))
        case(f"{fam}-{lay}-split5-scalar-reduce-132x130x1280", mode, lay, 132, 130, 1280, dict(family=fam, ns=5, slab_xcd=0),
             bias=True, bias2=True, relu=True, acc=True, mask=True, colsum=bool(ta))
    case(f"{fam}-tn-split128-rounded-to-121-128x128x65600", mode, "tn", 128, 128, 65600, dict(family=fam, ns=121, kchunk=544, slab_xcd=0), bias=True, colsum=True)
    # the 1-bit mask pair and the dropout epilogue (no split-K with the bits)
    case(f"{fam}-nt-bits-out-300x96x40" if fam == "gemm3" else "gemm-tt-bits-out-drop-300x96x40", mode, "nt" if fam == "gemm3" else "tt", 300, 96, 40,
         dict(family=fam, ns=1), bias=True, relu=True, bits="out", drop=fam != "gemm3")
    if fam == "gemm3":
        case("gemm3-nn-bits-in-300x96x40", mode, "nn", 300, 96, 40, dict(family=fam, ns=1), bits="in")
        case("gemm3-tn-bits-out-drop-300x96x40", mode, "tn", 300, 96, 40, dict(family=fam, ns=1), bias=True, relu=True, bits="out", drop=True)
        case("gemm3-nt-drop-300x96x40", mode, "nt", 300, 96, 40, dict(family=fam, ns=1), bias=True, relu=True, drop=True)
        case("gemm3b-nt-bits-out-256x256x96", mode, "nt", 256, 256, 96, dict(family="gemm3b", persistent=0, ns=1), bias=True, relu=True, bits="out")
        case("gemm3b-tn-bits-out-drop-256x256x96", mode, "tn", 256, 256, 96, dict(family="gemm3b", persistent=0, ns=1), bias=True, relu=True, bits="out", drop=True)
        case("gemm3b-nn-bits-in-512x256x96", mode, "nn", 512, 256, 96, dict(family="gemm3b", persistent=0, ns=1), bits="in")
        case("gemm3b-tt-drop-mask-256x512x96", mode, "tt", 256, 512, 96, dict(family="gemm3b", persistent=0, ns=1), bias=True, relu=True, drop=True, mask=True, colsum=True)
    case(f"{fam}-nt-split-wanted-no-workspace-128x128x2048", mode, "nt", 128, 128, 2048, dict(family=fam, ns=1, kchunk=2048, slab_xcd=0), bias=True, ws="null")
# bf16x6 mode on shapes its tiles do not take: split-K on the exact-fp32 kernel, scalar reduce and a short last slab
case("gemm-tn-x6-split5-scalar-reduce-132x130x1280", "bf16x6", "tn", 132, 130, 1280, dict(family="gemm", ns=5, slab_xcd=0), bias=True, bias2=True, relu=True, acc=True, colsum=True)
case("gemm-nt-x6-split4-short-last-slab-256x256x1030", "bf16x6", "nt", 256, 256, 1030, dict(family="gemm", ns=4, kchunk=288, slab_xcd=0, fast=0), bias=True)
case("gemm6e-tn-split-wanted-no-workspace-256x256x2048", "bf16x6", "tn", 256, 256, 2048, dict(family="gemm6e", ns=1, kchunk=2048, slab_xcd=0), colsum=True, ws="null")
case("gemm6e-nt-split-wanted-no-workspace-256x256x2048", "bf16x6", "nt", 256, 256, 2048, dict(family="gemm6e", ns=1, kchunk=2048, slab_xcd=0), bias=True, ws="null")
