"""The list-attention dispatch rules (include/rlt_hip.h) restated in Python, independently of
csrc/attention_dispatch.hip: tests/test_attention_plan.py compares every field of rlt_list_attention_plan with plan() below.

The rules are written the way the documents state them - a case analysis on (precision, head dim, list count, dropout, images) -
not as the sequence of overrides the C++ uses.  Switches: the environment variables of the attention family, as a dict of their
string values (absent = default)."""

GRID = ([(16, B) for B in (1, 64, 500, 511, 512, 576, 640)] + [(32, B) for B in (1, 130)] +
        [(64, B) for B in (1, 448, 512, 520, 576)] + [(128, 130)])
NON_SMALL24 = (1, 4096, 22, 64)          # (S, B, H, HD): B * 3 * H * HD >= 2^24, beyond the one-wavefront head-dim-64 backward kernels' loaders

# bytes of one tile record per family and head dim (64-row tiles; the pipelined kernels: 128-row tiles at head dim 16, 64-row at 64)
# bf16x3: hi + lo row images (64 x (HD + 8) bf16 each), hi + lo transposed images, either pair padded to 1 KiB, + 1 KiB of row data
X3_RECORD = {16: 6144 + 5120 + 1024, 32: 10240 + 9216 + 1024, 64: 18432 + 18432 + 1024}
X6_RECORD = {hd: 3 * 64 * (hd + 8) * 2 for hd in (16, 32, 64)}     # three bf16 planes of 64 rows, 8 columns of padding
X6N_RECORD, X6N_TILE = 12288, 128        # three bf16 planes of 128 rows x 16 columns: 12 LDS-DMA pieces of 1 KiB
X6H_RECORD, X6H_TILE = 24576, 64          # three planes of 64 rows x 64 columns: 24 pieces


def cdiv(a, b):
    return -(-a // b)


def _flag(sw, name, default=True):
    return default if name not in sw else int(sw[name]) != 0


def plan(S, B, H, HD, drop_p, have_images, precision, sw=None):
    sw = sw or {}
    drop = drop_p > 0
    p = dict(fwd="f32", fwd_fixup="none", dkv="f32", dq="f32", fwd_prepare=(), bwd_prepare=("delta",), dkv_prepare=(), dq_prepare=(),
             images_kind="none", images_retained=0, ws_kind="delta", images_bytes=0, flags_offset=0, flags_bytes=0, ws_extra_bytes=0)
    p["delta_bytes"] = cdiv(S * H * B * 4, 1024) * 1024
    pairs = S * H

    # which arithmetic: RLT_ATTN_MODE overrides the call's precision (and never selects bf16x6); head dim 128 is always exact fp32
    forced = sw.get("RLT_ATTN_MODE")
    if forced is not None:
        mode = "bf16x3" if forced in ("bf16x3", "1") else "fp32"
    else:
        mode = precision
    if HD == 128 or (mode == "bf16x6" and not _flag(sw, "RLT_ATTN6")):
        mode = "fp32"

    if mode == "bf16x3":
        p.update(images_kind="x3_qkv", images_retained=1, images_bytes=3 * pairs * cdiv(B, 64) * X3_RECORD[HD],
                 ws_kind="x3_do", ws_extra_bytes=pairs * cdiv(B, 64) * X3_RECORD[HD])
        if have_images:
            p.update(fwd="x3", dkv="x3", dq="x3", fwd_prepare=("q", "k", "v"), bwd_prepare=("do", "delta"))
        else:
            mode = "fp32"               # no images: the exact-fp32 kernels, the layout stays that of bf16x3

    if mode == "fp32":
        if HD == 16 and _flag(sw, "RLT_ATTN16"):
            p.update(fwd="f32_hd16", dkv="f32_hd16", dq="f32_hd16")
        elif HD == 128 or sw.get("RLT_DKV_OCC") == "1":
            p["dkv"] = "f32_occ1"
        if HD == 64 and _flag(sw, "RLT_ATTN_SB"):
            p["fwd"] = "f32_sb"
            if "RLT_ATTN_SB_DQ" in sw:
                p["dq"] = "f32_sb"

    if mode == "bf16x6":
        staged = _flag(sw, "RLT_ATTN6_IMG", False)
        if staged:
            p.update(images_kind="x6_qkv", images_retained=1, images_bytes=3 * pairs * cdiv(B, 64) * X6_RECORD[HD],
                     ws_kind="x6_do", ws_extra_bytes=pairs * cdiv(B, 64) * X6_RECORD[HD])
        img = staged and have_images
        if img:
            p.update(fwd_prepare=("q", "k", "v"), bwd_prepare=("do", "delta"))
        two_w = "x6_img" if img else "x6"
        if HD == 16:
            # attention6n.hip unless switched off or staging images (which only attention6.hip's kernels do)
            if _flag(sw, "RLT_A6N") and not img:
                two_w = "x6n_2w_seeded" if B >= 512 else "x6n_2w"
            pipe = (B >= 512 and not drop and not staged and
                    _flag(sw, "RLT_A6N") and _flag(sw, "RLT_A6N_1") and _flag(sw, "RLT_A6N_IMG"))
            p.update(fwd=two_w, dkv=two_w, dq=two_w)
            if pipe:
                blk = pairs * (cdiv(B, X6N_TILE) + 1) * X6N_RECORD
                p.update(dkv="x6n_pipe", dq="x6n_pipe", dkv_prepare=("q",), dq_prepare=("k", "v"), bwd_prepare=("do", "seeds", "delta"),
                         ws_kind="x6n_blocks", ws_extra_bytes=4 * blk + pairs * (cdiv(B, X6N_TILE) + 1) * 1024)
                if B % 128 == 0 and _flag(sw, "RLT_A6N_F1"):
                    p.update(images_kind="x6n_kv", flags_offset=2 * blk)
                    if have_images:
                        p.update(fwd="x6n_pipe", fwd_fixup="x6n_2w_seeded", fwd_prepare=("k", "v"))
        elif HD == 32:
            p.update(fwd=two_w, dkv=two_w, dq=two_w)
        else:
            small24 = B * 3 * H * HD < 2 ** 24
            pp = "x6_pp_img" if img else "x6_pp"
            p["fwd"] = pp if _flag(sw, "RLT_A6_PP") else two_w
            p["dkv"] = "x6_dkv1" if _flag(sw, "RLT_A6_DKV1") and small24 else two_w
            p["dq"] = "x6_dq1" if _flag(sw, "RLT_A6_DQ1") and small24 else two_w
            if B >= 512 and B % 64 == 0 and not staged and _flag(sw, "RLT_A6H"):       # train mode included
                p.update(images_kind="x6h_kv", flags_offset=2 * pairs * (cdiv(B, X6H_TILE) + 1) * X6H_RECORD)
                if have_images:
                    p.update(fwd="x6h_pipe", fwd_fixup="x6_pp", fwd_prepare=("k", "v"))
        if p["images_kind"] in ("x6n_kv", "x6h_kv"):
            p["flags_bytes"] = cdiv(pairs * cdiv(B, 256) * 4, 256) * 256
            p["images_bytes"] = p["flags_offset"] + p["flags_bytes"]

    p["ws_bytes"] = p["delta_bytes"] + p["ws_extra_bytes"]
    # _bwd_prepare asks for what it writes; _bwd_dkv / _bwd_dq for the whole layout, except a bf16x3-layout call without images
    p["ws_prepare_bytes"] = p["ws_bytes"] if len(p["bwd_prepare"]) > 1 else p["delta_bytes"]
    p["ws_part_bytes"] = p["delta_bytes"] if p["ws_kind"] == "x3_do" and not have_images else p["ws_bytes"]
    order = ("q", "k", "v", "do", "seeds", "delta")
    for f in ("fwd_prepare", "bwd_prepare", "dkv_prepare", "dq_prepare"):
        p[f] = tuple(sorted(p[f], key=order.index))
    return p
