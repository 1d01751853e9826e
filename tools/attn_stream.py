"""What the attention stream generators (gen_attention_w16.py, gen_attention_w32.py, gen_attention_w16l.py) share: the fragment-read scheduler
of one MFMA phase, the assertion of DESIGN 4.4 rule 3, a few instruction-stream helpers, the ablation filters and the `.inc` writer.

A plain module: it reads no environment variable and knows no register number.  A generator describes its stream as Phase objects (which
MFMAs, which fragments, what fills the gaps, where the DMA pieces, the barrier and the ring-slot advance go), hands emit_phase its own
fragment-register function fr(buffer position, pool, half) and gets asm lines back.
"""
import os
import sys


class Phase:
    """One phase of a stream, as data.
      mfma     [(MFMA text with a {fr} hole, index of the slot's fragment in `frags` | None)], one per slot
      frags    [[(address register, immediate), ...]] in order of first use: the ds_read_b128s that fill one fragment buffer (two for a
               32-byte fragment: half 0, half 1)
      pool     the buffer pool of every fragment (one name for all, or a list); bpos[f] = f's position in its pool, in order of first use
      rd       the slot behind whose MFMA fragment f is read, relative to the phase's slot 0 (negative: in the previous phase, counted
               from its end, or in front of the phase); default fu[f] - lookahead
      wg       wait granularity: one counted s_waitcnt every wg slots, for the fragments first used in those slots
      valu     per slot, the instructions that fill the gap behind its MFMA
      advance  [(address register, xor operand text)]: the ring-slot advance, placed behind the last own read through that register
      dma      {slot: (lines in front of the MFMA, the DMA instruction behind its reads)}
      barrier  None | ("before", slot, lines) — in front of everything of that slot | ("after", slot, lines) — behind its gap"""

    def __init__(self, name, mfma, frags, pool, wg, lookahead=None, rd=None):
        self.name, self.mfma, self.frags, self.wg, self.n = name, mfma, frags, wg, len(mfma)
        self.pool = [pool] * len(frags) if isinstance(pool, str) else pool
        self.valu, self.advance, self.dma, self.barrier = [[] for _ in range(self.n)], [], {}, None
        self.finish(lookahead, rd)

    def finish(self, lookahead, rd):
        nf = len(self.frags)
        self.fu = [min(i for i, (_, ff) in enumerate(self.mfma) if ff == f) for f in range(nf)]   # first / last slot that uses fragment f
        self.lu = [max(i for i, (_, ff) in enumerate(self.mfma) if ff == f) for f in range(nf)]
        assert self.fu == sorted(self.fu), self.fu
        self.bpos, cnt = [], {}
        for pl in self.pool:
            self.bpos.append(cnt.get(pl, 0))
            cnt[pl] = cnt.get(pl, 0) + 1
        self.count = cnt   # fragments per pool
        self.rd = rd if rd is not None else [self.fu[f] - lookahead for f in range(nf)]


class Ablation:
    """The parsed form of a generator's X string (timing experiments only: the streams compute wrong results).  words: a set of nomfma | nowait |
    novalu | noexp | halfreads | nolds | nodma | nobarrier (the last two are honoured by emit_phase) and whatever the generator asks for
    itself with `in`; drop: mnemonic prefixes of gap instructions to leave out; label: the generator's label prefix (novalu keeps labels)."""

    def __init__(self, words=(), drop=(), label="."):
        self.words, self.drop, self.label = set(words), tuple(drop), label

    def __contains__(self, word):
        return word in self.words

    def apply(self, i, pre, mf, rd, post):
        """slot i's lines in front of the MFMA, the MFMA, its reads, its gap -> the same, filtered"""
        if "halfreads" in self:
            rd = [r_ if k % 2 == 0 else "s_nop 0" for k, r_ in enumerate(rd)] if i % 4 < 2 else ["s_nop 0" for _ in rd]
        if "nomfma" in self:
            mf = "s_nop 0"
        if "nowait" in self:
            pre = [p_ for p_ in pre if not p_.startswith("s_waitcnt lgkmcnt")]
        if "novalu" in self:
            post = [p_ for p_ in post if p_.startswith(("s_", self.label, "v_xor", "v_cmp"))]
        if "noexp" in self:
            post = [p_.replace("v_exp_f32", "v_mov_b32") for p_ in post]
        if self.drop:
            post = [p_ for p_ in post if not p_.startswith(self.drop)]
        if "nolds" in self:
            rd = []
        return pre, mf, rd, post


def _reads(ph, fr, who):
    """[(slot, (key, destination registers, address register, immediate))] of ph's fragments in order; key = (who, f)"""
    return [(ph.rd[f], ((who, f), fr(ph.bpos[f], ph.pool[f], k if len(frag) > 1 else None), reg, imm))
            for f, frag in enumerate(ph.frags) for k, (reg, imm) in enumerate(frag)]


def early_reads(ph, fr):
    """the reads of ph's fragments that precede its slot 0 (what the previous phase's tail, or an own prefetch, issues), in order"""
    return [f"ds_read_b128 {b_}, {reg} offset:{imm}" for i, (_, b_, reg, imm) in _reads(ph, fr, 0) if i < 0]


def emit_phase(ph, nxt, fr, ablation, own_prefetch=False, drain=False):
    """asm lines of one phase.  `nxt` = the phase whose first fragments are fetched behind this phase's last MFMAs (None: none).
    Fragment f of a phase is read in the gap behind MFMA slot rd[f] (a negative slot: in the previous phase's tail, or in front of the
    phase when own_prefetch)."""
    o = [f"; ==== phase {ph.name}"]
    n, nf = ph.n, len(ph.frags)
    # ---- the read instructions of every gap, in stream order: key = (0, f) own fragment f, (1, f) the next phase's
    reads = [[] for _ in range(n)]
    early = []                               # read before slot 0 (previous phase's tail or own prefetch), in order
    for i, r in _reads(ph, fr, 0):
        (reads[i] if i >= 0 else early).append(r)
    own_last_read = max([g for g in range(n) if reads[g]], default=-1)
    if nxt is not None:
        for i, r in _reads(nxt, fr, 1):
            if i < 0:
                assert n + i > own_last_read, (ph.name, "next phase's reads must follow the own ones")
                reads[n + i].append(r)
    if own_prefetch:
        o += early_reads(ph, fr)
    # position of every read in issue order (early ones first); last[key] = position of that fragment's last read
    order = [key for (key, _, _, _) in early]
    issued_before_slot = [len(order)]
    for g in range(n):
        order += [key for (key, _, _, _) in reads[g]]
        issued_before_slot.append(len(order))   # issued before MFMA slot g + 1
    last = {key: k for k, key in enumerate(order)}
    # ---- ring-slot advance of the address registers: each register right behind the last own read that uses it (the next
    # phase's reads of that register come later by construction: asserted)
    adv_at = [[] for _ in range(n)]
    for reg, operand in ph.advance:
        own = [g for g in range(n) for (key, _, r_, _) in reads[g] if key[0] == 0 and r_ == reg]
        g_last = max(own, default=0)
        nxt_use = [g for g in range(n) for (key, _, r_, _) in reads[g] if key[0] == 1 and r_ == reg]
        assert all(g > g_last for g in nxt_use), (ph.name, reg, g_last, nxt_use)
        adv_at[g_last].append(f"v_xor_b32 {reg}, {operand}, {reg}")
    barrier = ph.barrier if ph.barrier and "nobarrier" not in ablation else (None, None, None)
    for i in range(n):
        text, f = ph.mfma[i]
        pre, dma = ph.dma.get(i, ([], None)) if "nodma" not in ablation else ([], None)
        pre = list(pre)
        # ---- counted wait (LDS reads retire in order) every wg-th slot, for every fragment first used in slots i .. i + wg - 1
        if i % ph.wg == 0:
            need = [f2 for f2 in range(nf) if i <= ph.fu[f2] < i + ph.wg]
            if need:
                younger = issued_before_slot[i] - last[(0, max(need))] - 1
                assert 0 <= younger <= 15, (ph.name, i, younger)
                pre.append(f"s_waitcnt lgkmcnt({younger})")
        mf = text.format(fr=fr(ph.bpos[f], ph.pool[f], None)) if f is not None else text
        rd = [f"ds_read_b128 {b_}, {reg} offset:{imm}" for (_, b_, reg, imm) in reads[i]]
        pre, mf, rd, post = ablation.apply(i, pre, mf, rd, adv_at[i] + ph.valu[i])
        o.append(f"; slot {i}")
        if barrier[:2] == ("before", i):
            o += barrier[2]
        o += pre + [mf] + rd
        if dma:
            o.append(dma)
        o += post
        if barrier[:2] == ("after", i):
            o += barrier[2]
    if drain:
        o += ["s_waitcnt lgkmcnt(0)", "s_nop 15", "s_nop 15", "s_nop 15"]
    return o


def check_rule3(seq, nbuf_of_pool, ordered=True):
    """DESIGN 4.4 rule 3.  Linearise a sequence of phases and assert that every read refills a buffer whose previous fragment's LAST MFMA sits
    strictly before the MFMA slot the read is issued behind (so a later MFMA has issued and the old operand has left the front of the matrix
    pipe), and — `ordered` — that reads are issued in stream order (False: several pools, each in its own order)."""
    base, last_user, prev_rd = 0, {}, None
    for ph in seq:
        for f in range(len(ph.frags)):
            rd = base + ph.rd[f]
            assert prev_rd is None or rd >= prev_rd or not ordered, ("stream order", ph.name, f)
            prev_rd = rd
            pb = (ph.pool[f], ph.bpos[f] % nbuf_of_pool[ph.pool[f]])
            assert last_user.get(pb, -10**9) < rd, ("rule 3", ph.name, f, pb, last_user.get(pb), rd)
            last_user[pb] = base + ph.lu[f]
        base += ph.n


def spread(plan, stream, first, last):
    """stream instructions over gaps first..last (inclusive), as evenly as integer division allows, in order"""
    n = last - first + 1
    for k, ins in enumerate(stream):
        plan[first + k * n // len(stream)].append(ins)


def max_chain(dst, regs):
    """dst = max(regs), a serial chain of v_max3 (the rare paths; the common path's maxima are trees, each generator's own)"""
    out = [f"v_max3_f32 {dst}, {regs[0]}, {regs[1]}, {regs[2]}"]
    k = 3
    while k + 1 < len(regs):
        out.append(f"v_max3_f32 {dst}, {dst}, {regs[k]}, {regs[k + 1]}")
        k += 2
    if k < len(regs):
        out.append(f"v_max_f32 {dst}, {dst}, {regs[k]}")
    return out


def lane_group_max(pm0, pm1, ta, tb):
    """pm0 / pm1 hold a per-lane maximum of query (block) 0 / 1; lanes n, n + 16, n + 32, n + 48 hold the same query.  Reduce over the four
    lane groups: after the first swap the lower half of the wave works on query 0 and the upper half on query 1; the last swap hands every
    lane both results, query 0's in ta and query 1's in tb."""
    return ["s_nop 1",
            f"v_permlane32_swap_b32 {pm0}, {pm1}",       # pm0 = [q0.r0, q0.r1, q1.r0, q1.r1]  pm1 = [q0.r2, q0.r3, q1.r2, q1.r3]
            "s_nop 1",
            f"v_max_f32 {ta}, {pm0}, {pm1}",
            f"v_mov_b32 {tb}, {ta}",
            "s_nop 1",
            f"v_permlane16_swap_b32 {ta}, {tb}",         # ta = [r0, r0, r2, r2]  tb = [r1, r1, r3, r3]
            "s_nop 1",
            f"v_max_f32 {ta}, {ta}, {tb}",
            f"v_mov_b32 {tb}, {ta}",
            "s_nop 1",
            f"v_permlane32_swap_b32 {ta}, {tb}",
            "s_nop 1"]


def scale_accumulators(regs, alpha, xt):
    """regs (accumulator registers) *= alpha, through the temporaries xt: a software pipeline of v_accvgpr_read / v_mul / v_accvgpr_write"""
    n = len(xt)
    out = [f"v_accvgpr_read_b32 {xt[0]}, {regs[0]}"]
    for r in range(len(regs)):
        if r + 1 < len(regs):
            out.append(f"v_accvgpr_read_b32 {xt[(r + 1) % n]}, {regs[r + 1]}")
        out.append(f"v_mul_f32 {xt[r % n]}, {xt[r % n]}, {alpha}")
        out.append(f"v_accvgpr_write_b32 {regs[r]}, {xt[r % n]}")
    return out


def rag_flag(tile_reg, flag, rag):
    """flag = 1 when the softmax of a phase works on the last tile (tile_reg == n - 1) and that tile is ragged (rag < 64 keys)"""
    return [f"s_cmp_eq_u32 {tile_reg}, %[ntm1]",
            f"s_cselect_b32 {flag}, 1, 0",
            f"s_cmp_lt_u32 {rag}, 64",
            f"s_cselect_b32 {flag}, {flag}, 0"]


def write_inc(path, banner, macro, lines, dump=None):
    """Write the stream as one C macro of string literals (lines that start with ';' are comments and stay out), the full text to `dump` when
    given, and report the counts on stderr."""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("".join(f"// {ln}\n" for ln in banner))
        f.write(f"#define {macro} \\\n")
        f.write(" \\\n".join('  "' + ln + '\\n\\t"' for ln in lines if not ln.startswith(";")))
        f.write("\n")
    if dump:
        with open(dump, "w") as f:
            f.write("\n".join(lines) + "\n")
    n_mfma = sum(1 for ln in lines if ln.startswith("v_mfma"))
    n_other = sum(1 for ln in lines if not ln.startswith(";") and not ln.startswith("v_mfma") and not ln.endswith(":"))
    print(f"{path}: {len(lines)} lines, {n_mfma} MFMAs, {n_other} other instructions", file=sys.stderr)
