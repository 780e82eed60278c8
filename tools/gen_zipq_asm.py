#!/usr/bin/env python3
"""Generates contractn_amd/csrc/kernels_zipq_asm.inc: the tiles of k_zipq_f32 (kernels_zipq.h) as inline-asm strings
with the phase-1 accumulators pinned to the 256 AGPRs - and kernels_zipqp_asm.inc, the same tiles for k_zipqp_f32
(kernels_zipqp.h; `selfadv`: the statements also advance the request cursor from tile to tile).

A tile is 128 MFMAs (8192 cycles of the matrix pipe) and one asm statement:

  phase 1 (P1)  8 k-steps of 16 MFMAs: T_q, T_q+1 [256 m1 x 32 u] += E^T X_q, E^T X_q+1 for 16 rows of k1.
                a[16 (8 q2 + mb) ...] is accumulator block (leg q2 of the pair, m1 block mb); 8 E + 2 X fragments.
  phase 2 (P2)  16 k-steps of 8 MFMAs: E'^T [256 n2 x 32 u] += Y_q^T T_q for the 32 rows m1 of block ms.
                k-step ks takes register ks of block (q2, ms) as its B operand straight from the AGPR; 8 Y fragments.

Every k-step issues its first MFMA, then the ds_read_b32 of the NEXT k-step's fragments into the other half of the
fragment double buffer (the last k-step: the next tile's first fragments, from the next ring stage), then its other
MFMAs, and waits lgkmcnt(0) at its end, when those reads are 7 or 15 MFMAs old.  Behind MFMA 56 sits the tile's
barrier (vmcnt(0): this wave's requests for the next tile, a tile old); behind MFMAs 66.. the wave's 8 LDS-DMA requests
for the tile after the next, one per MFMA.  The requests are the same text in every tile - two offset registers, two
base pointers and three increments, set up by the kernel - so a tile's text depends on its own kind only.

LDS image of a stage (32 KiB, 1 KiB per request, wave w fills [8 w, 8 w + 8) KiB):
  P1: per group of 4 rows k1 (= w): E rows 4 x 1 KiB, X_q rows 4 x 512 B, X_q+1 rows 4 x 512 B
  P2: row m1 (of 32) at m1 KiB
"""
import os

NMFMA = 128
BAR_AT = 56
REQ_AT = [66, 67, 68, 69, 70, 71, 73, 74]


def acc1(q2, mb):
    b = 16 * (8 * q2 + mb)
    return "a[%d:%d]" % (b, b + 15)


def e_off(kk, mb):
    return (kk // 2) * 8192 + 2 * (kk % 2) * 1024 + 128 * mb


def x_off(kk, q2):
    return (kk // 2) * 8192 + 2 * (kk % 2) * 512 + 2048 * q2


def y_off(ks, nb):
    return (8 * (ks // 4) + ks % 4) * 1024 + 128 * nb


def next_reads(nxt, buf):
    """The next tile's first fragments into buffer `buf` (0)."""
    if nxt == "P1":
        return ["ds_read_b32 %%[f%d], %%[nA] offset:%d" % (10 * buf + mb, e_off(0, mb)) for mb in range(8)] + \
               ["ds_read_b32 %%[f%d], %%[nB] offset:%d" % (10 * buf + 8 + q2, x_off(0, q2)) for q2 in range(2)]
    return ["ds_read_b32 %%[f%d], %%[nY] offset:%d" % (10 * buf + nb, y_off(0, nb)) for nb in range(8)]


def requests(selfadv=False):
    """`selfadv`: the statement finishes the cursor's step itself - a fourth add per offset register (%[ja] behind
    request 3, %[jb] behind request 7: the tile's step less the three row steps), so that between two tiles of one kind
    the kernel has nothing to recompute (k_zipqp_f32)."""
    out = []
    for i in range(8):
        r, s = ("ra", "sa") if i < 4 else ("rb", "sb")
        lines = ["s_mov_b32 m0, %[m0b]" if i == 0 else "s_add_u32 m0, m0, 0x400", "s_nop 0",
                 "global_load_lds_dwordx4 %%[%s], %%[%s]" % (r, s)]
        inc = {0: "ia", 1: "ia", 2: "ia", 4: "ib1", 5: "ib2", 6: "ib1"}.get(i)
        if selfadv and i in (3, 7):
            inc = "ja" if i == 3 else "jb"
        if inc:
            lines.append("v_add_u32 %%[%s], %%[%s], %%[%s]" % (r, inc, r))
        if i == 0:
            lines.insert(0, "s_mov_b32 %[keep], m0")
        if i == 7:
            lines.append("s_mov_b32 m0, %[keep]")
        out.append(lines)
    return out


def tile(kind, nxt, first=False, q2=0, ms=0, selfadv=False):
    mf, reads = [], {}          # MFMA texts; reads[i] = instructions behind MFMA i
    if kind == "P1":
        for kk in range(8):
            c, nx = kk & 1, (kk & 1) ^ 1
            for j in range(16):
                lq, mb = j // 8, j % 8
                src_c = "0" if (first and kk == 0) else acc1(lq, mb)
                mf.append("v_mfma_f32_32x32x2_f32 %s, %%[f%d], %%[f%d], %s" % (acc1(lq, mb), 10 * c + mb, 10 * c + 8 + lq, src_c))
            if kk < 7:
                reads[16 * kk] = ["ds_read_b32 %%[f%d], %%[vA] offset:%d" % (10 * nx + mb, e_off(kk + 1, mb)) for mb in range(8)] + \
                                 ["ds_read_b32 %%[f%d], %%[vB] offset:%d" % (10 * nx + 8 + l, x_off(kk + 1, l)) for l in range(2)]
            else:
                reads[16 * kk] = next_reads(nxt, nx)
        per = 16
    else:
        for ks in range(16):
            c, nx = ks & 1, (ks & 1) ^ 1
            for nb in range(8):
                mf.append("v_mfma_f32_32x32x2_f32 %%[c%d], %%[f%d], a%d, %%[c%d]" % (nb, 10 * c + nb, 16 * (8 * q2 + ms) + ks, nb))
            if ks < 15:
                reads[8 * ks] = ["ds_read_b32 %%[f%d], %%[vY] offset:%d" % (10 * nx + nb, y_off(ks + 1, nb)) for nb in range(8)]
            else:
                reads[8 * ks] = next_reads(nxt, nx)
        per = 8
    assert len(mf) == NMFMA
    req = dict(zip(REQ_AT, requests(selfadv)))
    out = []
    for i, m in enumerate(mf):
        out.append(m)
        out += reads.get(i, [])
        if i == BAR_AT:
            out += ["s_waitcnt vmcnt(0)", "s_barrier"]
        out += req.get(i, [])
        if i % per == per - 1:
            out.append("s_waitcnt lgkmcnt(0)")
    return out


def macro(name, lines):
    body = " \\\n".join('  "%s\\n\\t"' % l for l in lines)
    return "#define %s \\\n%s\n" % (name, body)


def emit(fname, prefix, hdr, selfadv=False):
    """One .inc file: the 19 tiles under `prefix`."""
    here = os.path.dirname(os.path.abspath(__file__))
    dst = os.path.join(here, "..", "contractn_amd", "csrc", fname)
    with open(dst, "w") as fh:
        fh.write(hdr)
        fh.write(macro(prefix + "_P1_FIRST", tile("P1", "P1", first=True, selfadv=selfadv)))
        fh.write(macro(prefix + "_P1_MID", tile("P1", "P1", selfadv=selfadv)))
        fh.write(macro(prefix + "_P1_LAST", tile("P1", "P2", selfadv=selfadv)))
        for q2 in range(2):
            for ms in range(8):
                nxt = "P1" if (q2, ms) == (1, 7) else "P2"
                fh.write(macro(prefix + "_P2_%d_%d" % (q2, ms), tile("P2", nxt, q2=q2, ms=ms, selfadv=selfadv)))
        fh.write("#define " + prefix + "_CLOBBERS \\\n  " + ", \\\n  ".join(
            ", ".join('"a%d"' % r for r in range(b, b + 16)) for b in range(0, 256, 16)) + "\n")
    print("wrote", os.path.normpath(dst))


emit("kernels_zipq_asm.inc", "CTN_ZQ", '''// GENERATED by tools/gen_zipq_asm.py - do not edit.  The tiles of k_zipq_f32 (kernels_zipq.h): 128 MFMAs each,
// phase-1 accumulators in a[0:255], fragment reads, the tile barrier and the LDS-DMA requests at fixed places.
''')
emit("kernels_zipqp_asm.inc", "CTN_ZQP", '''// GENERATED by tools/gen_zipq_asm.py - do not edit.  The tiles of k_zipqp_f32 (kernels_zipqp.h): those of
// kernels_zipq_asm.inc with a self-advancing request cursor (%[ja], %[jb]: the fourth add per offset register).
''', selfadv=True)
