#!/usr/bin/env python3
"""Generator of the tile bodies of the one-wavefront-per-SIMD head-dim-64 attention kernels on v_mfma_f32_16x16x32_bf16
(ranked-list-truncation_amd/csrc/attention6h_fwd1_body{,_drop}.inc; kernels in csrc/attention6h.hip).

The form is that of the head-dim-16 kernels (tools/gen_attn6n_body.py; both on tools/attn_pipe_sched.py): a tile body is NS slots, a
slot carries the MFMAs of the pipeline stages of different ITEMS of the 64-row tile.  What head dim 64 changes: a d-contracted
product is two k-steps of each of the six plane products (12 MFMAs per 16 x 16 tile, 24 per item), a d-indexed output four 16-row
blocks (24 MFMAs per item), so a slot is 52 (forward) / 76 (dQ) / 104 (dK+dV) MFMAs long and the vector work of an item (the same as at
head dim 16) fills a third of the gaps' capacity; the fragment registers of a 32-row block are SINGLE-buffered (a register is reloaded
in the gaps between its last use by own block NB - 1 and its first use by own block 0 of the next 32-row block: at least a quarter of
a slot).

    fwd (NB = 4, 52 per slot):  R1(s-2) x2 | O(s-3) x24 | R2(s-2) x2 | S(s) x24
    dq  (NB = 2, 76 per slot):  R1(s-2) x2 | O(s-3) x24 | R2(s-2) x2 | S(s) x24 | D(s) x24
    dkv (NB = 2, 104 per slot): RP1, RD1 (s-2) x2 each | OV(s-3) x24 | OK(s-3) x24 | RP2, RD2 (s-2) x2 each | S(s) x24 | D(s) x24

(S, D: the row products S = Q K^T and dP = dO V^T, index k = 12 kb + 2 product + k-step; R*: the matrix-pipe residuals of the
three-way split; O*: the list-contracted outputs, index k = 4 product + d block, the five small plane products into the second
accumulator.)  Dependences between MFMA results, chunks and MFMA operands - including the write-after-read ones of the register
rings and of the single-buffered fragments - are checked at generation time (verify()).

    python tools/gen_attn6h_body.py fwd      > ranked-list-truncation_amd/csrc/attention6h_fwd1_body.inc
    python tools/gen_attn6h_body.py fwd drop > ranked-list-truncation_amd/csrc/attention6h_fwd1_body_drop.inc

The dq and dkv modes are kept for the planned head-dim-64 backward in this form: no committed kernel uses them
(tests/test_generated_bodies.py pins their output).  fwd: the weights are exp2(score - fixed reference of the query) (seeded
scores), summed into the row's normaliser (e_sum; items of the drain tile multiply by a zero flag).  GEN_OMIT=name,name leaves the
calls of these names out, GEN_DMA_STEP sets the gaps between two staging pieces (timing experiments).
"""
import os
import sys

from attn_pipe_sched import MARGIN, PROD, RD_AHEAD, RING, WAR, Layout, Schedule, add_items, emit, parse_args

NB32 = 2                     # 32-row blocks per tile (tile = 64 rows)
COST = {"exp": 8, "mul": 4, "cvt": 5, "rd": 2, "ld": 3, "tb": 3, "drop": 16, "hc": 48}


def schedule(mode, drop=False, dma_step=5):
    lay = Layout(mode, 24, 4 if mode == "fwd" else 2, NB32)         # 4 / 2 16-row blocks of own rows per wavefront
    sch = Schedule(lay.G, lay.GS, COST)
    gap_of, GS, NS = lay.gap_of, lay.GS, lay.NS
    masks = {}

    def mask(i, kb, r, es):    # train mode: the dropout mask acts on the weight AFTER it went into the normaliser
        b32 = i // lay.NB
        masks[i, kb, r] = sch.add(f"ek{i}.{kb}{r}", [(f"e_drop({i % RING}, {i % lay.NB}, {kb}, {r}, {b32 & 1});", "drop")], 0,
                                  gap_of("R1", 0, i) - MARGIN - 1, [(es, 1)])
        return masks[i, kb, r]

    add_items(sch, lay, exp_lead=4 if drop else 2, after_sum=mask if drop else None)
    # LDS fragment reads of 32-row block b32 (single-buffered registers).  A register is free from its last use by the last own
    # block of the previous 32-row block (+ WAR) - for the first block of a tile that use lies in the previous body for the row
    # fragments (stage offset 0: from gap 0 on, i.e. behind the barrier that opens the tile) and up to three slots into this body
    # for the transposed fragments of the output stages - and must be issued RD_AHEAD gaps ahead of its first use.
    for b32 in range(NB32):
        first, prev_last = lay.first_item(b32), lay.last_item(b32 - 1)
        for stg, mat in lay.row_stages:
            for kb in range(2):
                for pl in range(3):
                    for ks in range(2):
                        # S / D index k = 12 kb + 2 product + k-step; A plane of the product = pl
                        fu, lu = lay.first_last(lambda k: k // 12 == kb and PROD[(k % 12) // 2][0] == pl and k % 2 == ks)
                        use = gap_of(stg, fu, first)
                        rel = gap_of(stg, lu, prev_last) + WAR if b32 >= 1 else 0
                        assert rel <= use - RD_AHEAD, ("row fragment window", stg, kb, pl, ks, rel, use)
                        sch.add(f"r{stg}{b32}.{kb}{pl}{ks}", [(f"rd_row({mat}, {kb}, {pl}, {ks}, {b32});", "rd")], rel, use - RD_AHEAD)
        for stg, mat in lay.out_stages:
            for pl in range(3):
                for db in range(4):
                    fu, lu = lay.first_last(lambda k: PROD[k // 4][0] == pl and k % 4 == db)
                    use = gap_of(stg, fu, first)
                    rel = max(0, gap_of(stg, lu, prev_last if b32 >= 1 else lay.last_item(NB32 - 1) - NS) + WAR)
                    assert rel <= use - RD_AHEAD, ("transposed fragment window", stg, pl, db, rel, use)
                    for half in range(2):
                        sch.add(f"t{stg}{b32}.{pl}{db}{half}", [(f"rd_tr({mat}, {pl}, {db}, {half}, {b32});", "rd")], rel, use - RD_AHEAD)
        if mode == "dkv":
            # -lse log2e / -delta of the block's 32 rows (the C operands of the first MFMA of S / dP): one float4 per 16-row block
            for kb in range(2):
                for which, stg in ((0, "S"), (1, "D")):
                    rel = gap_of(stg, 12 * kb, prev_last) + WAR if b32 >= 1 else 0
                    sch.add(f"tb{b32}.{kb}{which}", [(f"rd_tab({which}, {kb}, {b32});", "tb")], rel, gap_of(stg, 12 * kb, first) - RD_AHEAD)
    if drop:
        # column hashes of the block's 32 keys (one uint4 per 16-row block, double-buffered by block parity: the masks of a block's
        # last item are evaluated a slot after the next block's first score product) and the hash table of the NEXT tile's 64 keys
        for b32 in range(NB32):
            for kb in range(2):
                rel = GS if b32 == NB32 - 1 else 0        # (buffer 1's previous tenant: the previous tile's last block, masked up to slot 0)
                rd = sch.add(f"hc{b32}.{kb}", [(f"rd_hc({b32 & 1}, {kb}, {b32});", "tb")], rel, None)
                for i in range(lay.first_item(b32), lay.last_item(b32) + 1):
                    for r in range(4):
                        masks[i, kb, r].after.append((rd, RD_AHEAD))
        sch.add("hcol", [("st_hcol();", "hc")], 2 * GS, GS * (NS - 1))
    # staging of the next tile: LDS-DMA pieces of the pre-split tile records (2 images x 24 pieces of 1 KiB, a wavefront issues every
    # fourth one; dK+dV: + the piece of the rows' seeds): early in the body, so that they have landed long before the barrier
    dma = [sch.add(f"dma{j}", [(f"st_dma({j});", "ld")], GS // 2 + dma_step * j, GS * (NS - 2) + 10) for j in range(13 if mode == "dkv" else 12)]
    sch.solve()
    sch.verify()
    # the staging pieces carry their LDS base in M0, written by the first piece of a group: pieces in index order
    dma_at = [t.placed[0] for t in dma]
    assert dma_at == sorted(dma_at), dma_at
    emitted = [c for gap in sch.gaps for c, _k, _n, _g in gap if c.startswith("st_dma(")]
    assert emitted == [f"st_dma({j});" for j in range(len(dma))], emitted
    return sch, lay


def main():
    mode, drop = parse_args(sys.argv, "fwd", drop_modes=("fwd",))
    omit = set(filter(None, os.environ.get("GEN_OMIT", "").split(",")))
    sch, lay = schedule(mode, drop, int(os.environ.get("GEN_DMA_STEP", "5")))
    sys.stderr.write(sch.stats(mode))
    print(emit(sch, lay, f"gen_attn6h_body.py {mode}{' drop' if drop else ''}", "A6H_STAMP", omit=omit))


if __name__ == "__main__":
    main()
