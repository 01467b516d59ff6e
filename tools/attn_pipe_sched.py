"""What the generators of the pipelined attention tile bodies share (tools/gen_attn6n_body.py: head dim 16, tools/gen_attn6h_body.py:
head dim 64): the slot layout, the item pipeline, the gap scheduler, an independent check of its result, and the emitter.

A tile body is NS slots; a slot carries the MFMAs of the pipeline stages of different ITEMS (an item = one 32-row block of the tile
x one 16-row block of the wavefront's own rows = 512 scores).  Every MFMA is followed by a "gap" that the same wavefront fills with
vector work and LDS reads - a v_mfma_f32_16x16x32_bf16 hides about 8 cycles of vector issue behind it (tools/micro/mfma16_gap.hip:
two plain instructions, or one v_exp_f32, or a conversion + one plain).  The work is placed by list scheduling, earliest deadline
first, on the CYCLIC timeline of the body: the pipeline runs across tile boundaries, so work of the last three items of a tile sits
in the first slots of the next body, on the same ring of registers.  Nothing here is module-level state: a generator builds a
Layout and a Schedule, adds its tasks, calls solve(), verify() and emit().
"""
import os
import sys

RING = 4                     # item register sets
LAG = 2                      # gaps between an MFMA and the first vector read of its result
MARGIN = 2                   # a chunk that writes an MFMA operand sits at least this many gaps ahead of the MFMA
WAR = 2                      # a fragment register is rewritten at the earliest this many gaps behind the last MFMA that reads it
RD_AHEAD = 10                # an LDS read is issued at least this many gaps (100 - 160 cycles) ahead of the MFMA that takes its data
CAP = 8                      # vector-issue cycles a gap takes before the scheduler looks for another one
OFFSET = {"S": 0, "D": 0, "R1": 2, "R2": 2, "RP1": 2, "RD1": 2, "RP2": 2, "RD2": 2, "O": 3, "OV": 3, "OK": 3}      # stage -> item offset
# the six plane products, smallest first: (plane of the A operand, plane of the B operand); 0 = h, 1 = m, 2 = l
PROD = [(1, 1), (2, 0), (0, 2), (1, 0), (0, 1), (0, 0)]
# mode -> (stages of a slot in issue order, fresh operands that are split on the matrix pipe: P and / or dS).  S, D: the row products
# (scores, dP); R*: the residuals of the three-way split, two MFMAs each; O*: the list-contracted outputs
STAGES = {"fwd": (("R1", "O", "R2", "S"), ("P",)),
          "dq": (("R1", "O", "R2", "S", "D"), ("D",)),
          "dkv": (("RP1", "RD1", "OV", "OK", "RP2", "RD2", "S", "D"), ("P", "D"))}


def parse_args(argv, default, drop_modes=()):
    """(mode, drop) of the command line `tool [mode [drop]]`; anything else ends the run with a usage line"""
    mode = argv[1] if len(argv) > 1 else default
    drop = argv[2:] == ["drop"]
    if mode not in STAGES or len(argv) > 3 or (argv[2:] and not drop) or (drop and mode not in drop_modes):
        forms = [m + (" [drop]" if m in drop_modes else "") for m in STAGES]
        sys.exit(f"usage: {os.path.basename(argv[0])} [{' | '.join(forms)}]")
    return mode, drop


class Layout:
    """Slots of one mode: n MFMAs per row / output stage, nb 16-row blocks of own rows, nb32 32-row blocks per tile."""

    def __init__(self, mode, n, nb, nb32):
        self.mode, self.n, self.NB, self.NB32, self.NS = mode, n, nb, nb32, nb * nb32        # NS: slots (= items) per tile body
        names, self.mats = STAGES[mode]
        self.layout = [(s, k) for s in names for k in range(2 if s.startswith("R") else n)]
        self.GS = len(self.layout)             # gaps per slot
        self.G = self.GS * self.NS             # gaps per body
        self.pos = {sk: g for g, sk in enumerate(self.layout)}
        self.row_stages = (("S", 0), ("D", 1))[:1 if mode == "fwd" else 2]           # (stage, matrix whose rows it reads)
        # (stage, matrix whose transpose it reads) - fwd: V^T; dq: K^T; dkv: dO^T for dV, Q^T for dK
        self.out_stages = {"fwd": (("O", 1),), "dq": (("O", 0),), "dkv": (("OV", 1), ("OK", 0))}[mode]

    def gap_of(self, stg, k, item):
        """absolute gap (item 0's S stage starts in slot 0) of MFMA k of stage `stg` of `item`"""
        return (item + OFFSET[stg]) * self.GS + self.pos[(stg, k)]

    def r_stage(self, m, lvl):
        return f"R{lvl}" if len(self.mats) == 1 else f"R{m}{lvl}"

    def o_stage(self, m):
        return "O" if len(self.mats) == 1 else ("OV" if m == "P" else "OK")

    def first_item(self, b32):
        return b32 * self.NB

    def last_item(self, b32):
        return b32 * self.NB + self.NB - 1

    def first_last(self, pred):
        """first and last index k within a row / output stage of the MFMAs that satisfy pred(k)"""
        ks = [k for k in range(self.n) if pred(k)]
        return ks[0], ks[-1]


class Task:
    def __init__(self, name, chunks, release, deadline, after=()):
        self.name, self.chunks, self.release, self.deadline = name, chunks, release, deadline    # chunks: (call, kind)
        self.after = list(after)      # (task, lag): first chunk at gap >= last chunk of task + lag
        self.placed = []              # absolute gap of every chunk


class ScheduleError(Exception):
    pass


class Schedule:
    """Tasks on a cyclic timeline of G gaps (GS per slot); cost: vector-issue cycles per kind of chunk."""

    def __init__(self, G, GS, cost):
        self.G, self.GS, self.cost = G, GS, cost
        self.tasks = []
        self.capv = [CAP] * G
        self._clear()

    def add(self, name, chunks, release, deadline, after=()):
        t = Task(name, chunks, release, deadline, after)
        self.tasks.append(t)
        return t

    def _clear(self):
        self.used = [0] * self.G
        self.gaps = [[] for _ in range(self.G)]       # per gap: (call, kind, task name, absolute gap)
        for t in self.tasks:
            t.placed = []

    def _place(self, t):
        G, used = self.G, self.used
        lo = t.release
        for dep, lag in t.after:
            assert dep.placed, (t.name, dep.name)
            lo = max(lo, dep.placed[-1] + lag)
        g = lo
        for call, kind in t.chunks:
            c = self.cost[kind]
            # a gap takes chunks up to its capacity (a chunk larger than that: a gap of its own) and at most one exp
            while used[g % G] + c > max(self.capv[g % G], c) or (kind == "exp" and any(x[1] == "exp" for x in self.gaps[g % G])):
                g += 1
                if t.deadline is not None and g > t.deadline:
                    return False
            used[g % G] += c
            self.gaps[g % G].append((call, kind, t.name, g))
            t.placed.append(g)
            g += 1
        return t.deadline is None or t.placed[-1] <= t.deadline

    def run(self):
        """dependency-respecting EDF: repeatedly take the unplaced task with the earliest deadline whose dependences are placed;
        returns the task that missed its deadline, or None"""
        self._clear()
        pending = list(self.tasks)
        while pending:
            ready = [t for t in pending if all(d.placed for d, _ in t.after)]
            t = min(ready, key=lambda t: (t.deadline if t.deadline is not None else 1 << 30, t.release))
            if not self._place(t):
                return t
            pending.remove(t)
        return None

    def solve(self):
        """run(); while a task misses its deadline, let the gaps of its window (and six ahead of it) take one more cycle"""
        for _ in range(400):
            miss = self.run()
            if miss is None:
                return
            lo = miss.release
            for dep, lag in miss.after:
                lo = max(lo, (dep.placed[-1] if dep.placed else 0) + lag)
            hi = miss.deadline if miss.deadline is not None else lo + self.GS
            for g in range(min(lo, hi) - 6, hi + 1):
                self.capv[g % self.G] += 1
        sys.exit(f"no schedule: {miss.name} (release {miss.release}, deadline {miss.deadline})")

    def verify(self):
        verify(self.tasks, self.capv, self.cost)

    def stats(self, mode):
        used, G = self.used, self.G
        return (f"{mode}: {G} gaps, capacity {CAP}..{max(self.capv)} cycles per gap, mean load {sum(used) / G:.1f}, max {max(used)}, "
                f"{sum(1 for u in used if u > CAP)} gaps over {CAP} cycles (sum of the excess {sum(max(0, u - CAP) for u in used)})\n")


def verify(tasks, capv, cost):
    """The dependences of a placed schedule, checked from the tasks' gaps alone (not from the scheduler's books): release, `after`
    lags, deadline, capacity of every gap of the cyclic timeline, one exp per gap.  Raises ScheduleError."""
    G = len(capv)
    load, exps, count = [0] * G, [0] * G, [0] * G
    for t in tasks:
        p = t.placed
        if len(p) != len(t.chunks) or any(b <= a for a, b in zip(p, p[1:])):
            raise ScheduleError(f"{t.name}: chunks at {p}")
        if p[0] < t.release:
            raise ScheduleError(f"{t.name}: gap {p[0]} before its release {t.release}")
        for dep, lag in t.after:
            if not dep.placed or p[0] < dep.placed[-1] + lag:
                raise ScheduleError(f"{t.name}: gap {p[0]} less than {lag} behind {dep.name} at {dep.placed}")
        if t.deadline is not None and p[-1] > t.deadline:
            raise ScheduleError(f"{t.name}: gap {p[-1]} behind its deadline {t.deadline}")
        for g, (_call, kind) in zip(p, t.chunks):
            load[g % G] += cost[kind]
            count[g % G] += 1
            exps[g % G] += kind == "exp"
    for g in range(G):
        if load[g] > capv[g] and count[g] > 1:
            raise ScheduleError(f"gap {g}: {load[g]} cycles of {capv[g]}")
        if exps[g] > 1:
            raise ScheduleError(f"gap {g}: {exps[g]} exp chunks")


def add_items(sch, lay, exp_lead=2, after_sum=None):
    """The element-wise pipeline of every item of a tile body, per score register (kb, r): ep = exp2 of the score; forward: es = the
    weight into the normaliser, backward: ed = P (dP - delta); then per split matrix the conversions c_pk of the three planes, four
    register pairs each.  after_sum(i, kb, r, es) may add a forward task between the sum and the conversion and returns it; the exp
    then leaves room for it: exp_lead gaps between its deadline and that of the conversion."""
    gap_of, n = lay.gap_of, lay.n
    first_l = min(p for p, (_a, b) in enumerate(PROD) if b == 2) * (n // 6)     # first output product that reads plane l (B plane 2)
    for i in range(lay.NS):
        it, nb = i % RING, i % lay.NB
        src = {"P": {}, "D": {}}
        # one gap per link of the chain exp -> (mul ->) conversion ahead of the first residual MFMA
        ep_dl = gap_of(lay.r_stage("P", 1), 0, i) - MARGIN - (1 if len(lay.mats) == 2 else exp_lead)
        for kb in range(2):
            for r in range(4):
                ep = sch.add(f"ep{i}.{kb}{r}", [(f"e_exp({it}, {kb}, {r});", "exp")], gap_of("S", (kb + 1) * n // 2 - 1, i) + LAG, ep_dl)
                src["P"][kb, r] = ep
                if lay.mode == "fwd":      # the weight into the normaliser of own block nb (any time before the registers turn into residuals)
                    es = sch.add(f"es{i}.{kb}{r}", [(f"e_sum({it}, {nb}, {kb}, {r});", "mul")], 0, gap_of("R1", kb, i) - 1, [(ep, 1)])
                    if after_sum:
                        src["P"][kb, r] = after_sum(i, kb, r, es)
                else:
                    src["D"][kb, r] = sch.add(f"ed{i}.{kb}{r}", [(f"e_mul({it}, {kb}, {r});", "mul")], gap_of("D", (kb + 1) * n // 2 - 1, i) + LAG,
                                              gap_of(lay.r_stage("D", 1), 0, i) - MARGIN - 1, [(ep, 1)])
        for m in lay.mats:
            r1, r2, out, mi = lay.r_stage(m, 1), lay.r_stage(m, 2), lay.o_stage(m), 0 if m == "P" else 1
            for j in range(4):         # plane h: from the fp32 values
                kb, rr = j >> 1, j & 1
                sch.add(f"c0{m}{i}.{j}", [(f"c_pk({it}, {mi}, 0, {j});", "cvt")], 0, gap_of(r1, 0, i) - MARGIN,
                        [(src[m][kb, 2 * rr], 1), (src[m][kb, 2 * rr + 1], 1)])
            for j in range(4):         # plane m: from the first residual
                sch.add(f"c1{m}{i}.{j}", [(f"c_pk({it}, {mi}, 1, {j});", "cvt")], gap_of(r1, j >> 1, i) + LAG, gap_of(r2, 0, i) - MARGIN)
            # plane l: from the second residual, ahead of the first output product that reads it; the item's fp32 registers are
            # rewritten by the first row product of item i + RING
            dl = min(gap_of(out, first_l, i) - MARGIN, gap_of("S", 0, i + RING) - 1)
            for j in range(4):
                sch.add(f"c2{m}{i}.{j}", [(f"c_pk({it}, {mi}, 2, {j});", "cvt")], gap_of(r2, j >> 1, i) + LAG, dl)


def late_name(call):
    """forward: chunks of a tile's last items that land in the NEXT body get their own names - the previous tile is always a live
    one, except in the first body, where there is none: there they belong to no tile and e_exp_p must produce a zero weight"""
    return call.replace("e_sum(", "e_sum_p(").replace("e_exp(", "e_exp_p(")


def emit(sch, lay, tool, stamp, frag_buf=None, omit=()):
    """The body: per slot a comment and the stamp macro, per gap one line `MFMA GAP_END; work GAP_END;` (GAP_END = sched_barrier keeps
    hipcc from reordering).  frag_buf(item): fragment buffer that the row and output products name as their last argument, if any."""
    out = [f"// generated by tools/{tool} - do not edit"]
    for s in range(lay.NS):
        out.append(f"// slot {s}")
        out.append(f"{stamp}({s});")
        for g0, (stg, k) in enumerate(lay.layout):
            i = s - OFFSET[stg]                 # item (negative: of the previous tile - same ring slot, same own-row block)
            it, nb = i % RING, i % lay.NB
            fb = f", {frag_buf(i)}" if frag_buf else ""
            if stg in ("S", "D"):
                call = f"m_{stg.lower()}({it}, {nb}, {k}{fb});"
            elif stg.startswith("R"):
                which = 0 if lay.mode == "fwd" else (1 if stg in ("R1", "R2", "RD1", "RD2") else 0)
                call = f"m_r({it}, {which}, {1 if stg.endswith('1') else 2}, {k});"
            else:
                which = 0 if lay.mode == "fwd" else {"O": 1, "OV": 0, "OK": 1}[stg]
                call = f"m_o({it}, {nb}, {which}, {k}{fb});"
            calls = [late_name(c) if lay.mode == "fwd" and g >= lay.G else c for c, _k, _n, g in sch.gaps[s * lay.GS + g0]]
            work = " ".join(c for c in calls if c.split("(")[0] not in omit)
            out.append(f"{call} GAP_END; {work} GAP_END;".replace("  ", " "))
    out.append(f"// {sum(1 for x in sch.gaps if x)} of {lay.G} gaps carry vector work; capacity {max(sch.capv)} cycles per gap")
    return "\n".join(out)
