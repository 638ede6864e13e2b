"""Seeded PDSCH encoder inputs that reach every lifting size a single-codeblock transport block selects, in both base
graphs, on every edge of the rate matcher's geometry: the regime grid of tests/test_pdsch_encoder_regimes_oracle.py
(the classes the inputs reach and the hand-made errors they tell from a right encoder, with the oracle alone),
tests/test_oracle_vs_reference.py and tests/test_golden.py (the oracle held to the reference on them) and
tests/test_pdsch_encoder_regimes_gpu.py (both HIP kernels held to the oracle on them).

geometry() and census() restate bit selection and interleaving from TS 38.212 section 5.4.2 and the reference
(ldpc_rate_matcher_impl.cpp:95-150) and classify a codeblock of a TB configuration; they share no code with the plan.

Grid (build_grid): per shape (base graph, Z) two TBs, the smallest and the largest byte count that select the shape as
one codeblock (most and fewest fillers); per TB the cells rv 0..3 x circular buffer (KINDS); per cell the rate-matched
lengths of ROLES, placed relative to the cell's geometry. One layer, so E = Qm R is free. The roles are rotated over the
cells: every role of a shape is emitted REPS times (once per Qm on the packed shapes), first with Qm = 1, which hits the
edge exactly, then with the two multiples of a rotating Qm that straddle it. A last pass adds, per shape (and per Qm on a
packed shape), one case for every class (CLASSES and PAIRS) that some cell reaches and the rotation missed.

Plain numpy; nothing here calls the oracle except expected() and its cache."""
import numpy as np

from oracle_lib import BG_K, BG_N_SHORT
from srsgpu import sch

# TS 38.212 Table 5.4.2.1-2: k0 = floor(SHIFT * Ncb / (N_SHORT * Zc)) * Zc.
SHIFT = {1: (0, 17, 33, 56), 2: (0, 13, 25, 43)}
QMS = (1, 2, 4, 6, 8)
KINDS = ("full", "lbrm_two_thirds", "lbrm_shortest", "lbrm_multiple")
CLASSES = ["wrap", "multi_wrap", "exact_fit", "k0_in_filler", "lbrm", "ncb_partial_column", "ends_in_systematic",
           "ends_on_column_last_bit", "ends_on_column_first_bit", "window_straddles_ninfo", "window_straddles_wrap",
           "group8"]
PACKED_ONLY = ("window_straddles_ninfo", "window_straddles_wrap", "group8")
# Conjunctions the hand-made errors of the oracle test need on every shape that has both parts.
PAIRS = {"partial_and_multi_wrap": ("ncb_partial_column", "multi_wrap"), "filler_skip_moves_n_ext": ("n_ext_needs_filler_skip",
                                                                                          "n_ext_needs_filler_skip")}
ROLES = ["fit-1", "fit", "fit+1", "multi", "sys", "sys+1",
         "ext0_last", "ext0_next", "ext1_last", "ext1_next", "ext2_last", "ext2_next", "mid_last", "mid_next",
         "end_last", "end_next", "start_last", "start_next"]
REPS = 2
GOLDEN_Z = {1: [2, 3, 7, 15, 32, 64, 120, 208, 288, 384], 2: [4, 7, 15, 32, 64, 72, 120, 208, 288, 384]}
# Multi-codeblock TBs: (TB bytes, base graph, codeblocks, Z). Two and three codeblocks start at Z = 208.
MULTI = [(1101, 1, 2, 208), (1137, 1, 2, 224), (2106, 1, 3, 288), (2112, 1, 3, 288),
         (480, 2, 2, 208), (633, 2, 2, 288), (954, 2, 3, 288), (1068, 2, 3, 288)]


def geometry(bg, Z, filler, rv, Nref):
    """The circular buffer of a codeblock: N bits without the 2 Z punctured ones, nsys systematic positions of which
    the last `filler` are fillers (ninfo before them), Ncb buffer positions, the start k0 and, counting the positions
    that are no fillers only, the start v0 and the buffer length V. A k0 inside the filler range starts at the first
    position behind it."""
    K, N = BG_K[bg], BG_N_SHORT[bg] * Z
    nsys = (K - 2) * Z
    ninfo = nsys - filler
    Ncb = min(Nref, N) if Nref > 0 else N
    k0 = SHIFT[bg][rv] * Ncb // N * Z
    v0 = k0 if k0 < ninfo else ninfo if k0 < nsys else k0 - filler
    return dict(bg=bg, Z=Z, K=K, filler=filler, rv=rv, N=N, nsys=nsys, ninfo=ninfo, Ncb=Ncb, k0=k0, v0=v0,
                V=Ncb - filler)


def windows(E, qm, g0):
    """The e windows (first selection index, length) that rate_match_packed's aligned path reads for a codeblock whose
    output starts at codeword bit g0: 32 / Qm bits per bit row and whole output word, and for Qm 8 at a word-aligned
    offset 32 bits per bit row and whole group of 32 symbols, the words behind the groups as before."""
    if qm not in (1, 2, 4, 8) or g0 % qm:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    R = E // qm
    t0 = np.arange((-g0) % 32, E - 31, 32, dtype=np.int64)
    rows = np.arange(qm, dtype=np.int64)[:, None] * R
    start, length = [], []
    if qm == 8 and g0 % 32 == 0:
        ng = R // 32
        start.append((rows + 32 * np.arange(ng, dtype=np.int64)[None, :]).ravel())
        length.append(np.full(8 * ng, 32, np.int64))
        t0 = t0[t0 >= 256 * ng]
    start.append((rows + (t0 // qm)[None, :]).ravel())
    length.append(np.full(qm * t0.size, 32 // qm, np.int64))
    return np.concatenate(start), np.concatenate(length)


def codeblock(case, cb=0):
    """(segmentation, codeblock `cb`) of a TB configuration."""
    seg = sch.segment(case["tb_bytes"] * 8, case["bg"], case["qm"], case["layers"], case["nsym"])
    return seg, seg.codeblocks[cb]


def is_packed(seg, cb):
    """The packed kernel takes a codeblock when Z % 32 == 0 and its TB data, and the span its CRC covers, are whole
    bytes at a byte offset."""
    last = cb.index == seg.nof_segments - 1
    data = cb.nof_info_bits + (seg.nof_tb_crc_bits if last else 0)
    covered = data + (seg.zero_pad if last else 0)
    return (seg.lifting_size % 32 == 0 and cb.tb_offset % 8 == 0 and data % 8 == 0 and
            (seg.cb_crc_bits == 0 or covered % 8 == 0))


def census(case, cb=0):
    """What codeblock `cb` of a TB configuration reaches: its geometry, the highest full-codeblock position the
    selection reads (punctured columns counted) and the extension rows (columns behind the K + 4 of the core) that
    holds, the kernel the plan picks, and one flag per class of CLASSES."""
    seg, c = codeblock(case, cb)
    g = geometry(case["bg"], seg.lifting_size, seg.nof_filler_bits, case["rv"], case["Nref"])
    Z, K, F, E, qm = g["Z"], g["K"], g["filler"], c.rm_length, case["qm"]
    v0, V, ninfo = g["v0"], g["V"], g["ninfo"]

    def full(v):
        return v + 2 * Z + (F if v >= ninfo else 0)

    wrap = E > V - v0
    top = g["Ncb"] - 1 + 2 * Z if E >= V - v0 else full(v0 + E - 1)
    end = full((v0 + E - 1) % V)
    packed = is_packed(seg, c)
    out = dict(g, E=E, qm=qm, R=E // qm, g0=c.cw_offset, top=top, n_ext=max(0, top // Z - (K + 4) + 1),
               kernel="packed" if packed else "byte", end=end)
    out["wrap"] = wrap
    out["multi_wrap"] = E >= 2 * V
    out["exact_fit"] = E == V - v0
    out["k0_in_filler"] = ninfo <= g["k0"] < g["nsys"]
    out["lbrm"] = g["Ncb"] < g["N"]
    out["ncb_partial_column"] = g["Ncb"] % Z != 0
    out["ends_in_systematic"] = v0 + E - 1 < ninfo
    out["ends_on_column_last_bit"] = not wrap and end % Z == Z - 1
    out["ends_on_column_first_bit"] = not wrap and end % Z == 0
    # The extension rows counted from the last selected position without the fillers it skipped would be too few.
    out["n_ext_needs_filler_skip"] = E < V - v0 and max(0, (v0 + E - 1 + 2 * Z) // Z - (K + 4) + 1) < out["n_ext"]
    straddle_ninfo = straddle_wrap = False
    if packed:
        n, L = windows(E, qm, c.cw_offset)
        v = (v0 + n) % V
        straddle_wrap = bool((v + L > V).any())
        straddle_ninfo = F > 0 and bool(((v < ninfo) & (v + L > ninfo)).any())
    out["window_straddles_ninfo"] = straddle_ninfo
    out["window_straddles_wrap"] = straddle_wrap
    out["group8"] = packed and qm == 8 and c.cw_offset % 32 == 0 and E // 8 >= 32 and (E // 8) % 32 != 0
    for name, (a, b) in PAIRS.items():
        out[name] = bool(out[a] and out[b])
    return out


def single_codeblock_shapes():
    """{(bg, Z): (smallest, largest TB bytes)} of the shapes a byte-sized TB of one codeblock selects."""
    shapes = {}
    for bg in (1, 2):
        nb = 1
        while True:
            seg = sch.segment(nb * 8, bg, 1, 1, 8)
            if seg.nof_segments > 1:
                break
            lo, _ = shapes.get((bg, seg.lifting_size), (nb, nb))
            shapes[bg, seg.lifting_size] = (lo, nb)
            nb += 1
    return shapes


def nref_of(kind, bg, Z):
    """The limited-buffer size of a kind: about two thirds into the parity part and no multiple of Z, the shortest
    buffer of the grid (half a column and a bit behind the systematic part), and a multiple of Z."""
    K, N = BG_K[bg], BG_N_SHORT[bg] * Z
    nsys = (K - 2) * Z
    if kind == "full":
        return 0
    if kind == "lbrm_two_thirds":
        n = nsys + 2 * (N - nsys) // 3
        return n + 1 if n % Z == 0 else n
    if kind == "lbrm_shortest":
        return nsys + Z // 2 + 1
    return nsys + (N - nsys) // Z // 2 * Z


def targets(g, salt):
    """{role: rate-matched length in bits} of a cell's geometry. Column roles end on the last bit of a lifted column
    (`_last`) and on the first bit of the one behind it (`_next`): the columns that make 0, 1 and 2 extension rows
    needed, one in the middle of the extension part that moves with `salt`, the buffer's last whole column, and the
    column the selection starts in; only where the selection gets there before it wraps."""
    Z, K, F, v0, V, ninfo, nsys, Ncb = (g[k] for k in ("Z", "K", "filler", "v0", "V", "ninfo", "nsys", "Ncb"))
    t = {"fit-1": V - v0 - 1, "fit": V - v0, "fit+1": V - v0 + 1, "multi": 2 * V + Z + 1}
    if v0 < ninfo:
        t["sys"], t["sys+1"] = ninfo - v0, ninfo - v0 + 1

    def length_to(p):
        """Bits selected up to buffer position p, or None when p is a filler, before the start or outside."""
        if ninfo <= p < nsys or p >= Ncb:
            return None
        u = p if p < ninfo else p - F
        return u - v0 + 1 if u >= v0 else None

    end_col = Ncb // Z + 1  # full-codeblock index of the buffer's last whole column
    cols = {"ext0": K + 3, "ext1": K + 4, "ext2": K + 5, "end": end_col, "start": g["k0"] // Z + 2}
    if end_col - 1 > K + 6:
        cols["mid"] = K + 6 + salt % (end_col - 1 - (K + 6))
    for name, c in cols.items():
        if c > end_col:
            continue
        for suffix, p in (("_last", (c - 1) * Z - 1), ("_next", (c - 1) * Z)):
            n = length_to(p)
            if n is not None:
                t[name + suffix] = n
    return {k: n for k, n in t.items() if n >= 1}


def can_occur(cls, Z, qm):
    """False for the (class, Qm) pairs that no length reaches: the window classes belong to Qm 1, 2, 4 and 8, group8
    to Qm 8, and with an even Z (starts and columns multiples of Z, filler counts multiples of 8) a length up to a
    column's first bit is odd."""
    if cls == "group8":
        return qm == 8
    if cls.startswith("window"):
        return qm != 6
    return not (cls == "ends_on_column_first_bit" and Z % 2 == 0 and qm % 2 == 0)


def _lengths(target, qm):
    """Qm 1: the target. Else the two multiples of Qm that straddle it."""
    if qm == 1:
        return [target]
    lo = target // qm * qm
    return [e for e in (lo, lo + qm) if e > 0]


def _case(bg, Z, tbi, nb, rv, kind, role, qm, E):
    return dict(bg=bg, Z=Z, tb_index=tbi, tb_bytes=nb, rv=rv, kind=kind, role=role, qm=qm, layers=1, nsym=E // qm,
                Nref=nref_of(kind, bg, Z))


def transport_block(case):
    """The TB's bytes: seeded by its size and base graph, its last bytes set (a byte masked off at the end shows)."""
    tb = np.random.default_rng([7300, case["bg"], case["tb_bytes"]]).integers(0, 256, case["tb_bytes"]).astype(np.uint8)
    tb[-2:] |= 0x81
    return tb


def build_grid(sizes=None):
    """The grid's TB configurations, shape by shape, for the lifting sizes `sizes` (all). A shape's cases depend on the
    shape only, so a subset of sizes yields the same cases as the whole grid."""
    cases = []
    for si, ((bg, Z), tb_sizes) in enumerate(sorted(single_codeblock_shapes().items())):
        if sizes is not None and Z not in sizes:
            continue
        cells = [(tbi, nb, rv, kind) for tbi, nb in enumerate(tb_sizes) for rv in range(4) for kind in KINDS]
        geo, k0_in_filler = [], False
        for ci, (tbi, nb, rv, kind) in enumerate(cells):
            g = geometry(bg, Z, sch.segment(nb * 8, bg, 1, 1, 8).nof_filler_bits, rv, nref_of(kind, bg, Z))
            geo.append(targets(g, si + ci))
            k0_in_filler = k0_in_filler or g["ninfo"] <= g["k0"] < g["nsys"]
        mine = []
        for ti, role in enumerate(ROLES):
            feasible = [ci for ci in range(len(cells)) if role in geo[ci]]
            # Qm 1 first; then every other Qm on a packed shape, else REPS - 1 of them, rotated.
            qms = QMS if Z % 32 == 0 else (1,) + tuple(QMS[1 + (si + ti + r) % 4] for r in range(REPS - 1))
            for r, qm in enumerate(qms):
                if not feasible:
                    break
                ci = feasible[(5 * si + 3 * ti + 7 * r) % len(feasible)]
                tbi, nb, rv, kind = cells[ci]
                mine += [_case(bg, Z, tbi, nb, rv, kind, role, qm, E) for E in _lengths(geo[ci][role], qm)]
        # Classes some cell of the shape reaches and the rotation missed: the first candidate that has them. On a
        # packed shape, per Qm.
        def candidates(qms):
            for ci, (tbi, nb, rv, kind) in enumerate(cells):
                for role, target in geo[ci].items():
                    for qm in qms:
                        for E in _lengths(target, qm):
                            yield _case(bg, Z, tbi, nb, rv, kind, role, qm, E)

        reached = {(k, c["qm"]) for c in mine for k, hit in census(c).items() if hit is True}
        for cls in CLASSES + list(PAIRS):
            if (cls in PACKED_ONLY and Z % 32) or (cls == "k0_in_filler" and not k0_in_filler):
                continue
            for qms in ([(qm,) for qm in QMS] if Z % 32 == 0 and cls in CLASSES else [QMS]):
                if any((cls, qm) in reached for qm in qms) or not any(can_occur(cls, Z, qm) for qm in qms):
                    continue
                found = next((c for c in candidates(qms) if census(c)[cls]), None)
                if found is not None:
                    mine.append(found)
                    reached |= {(k, found["qm"]) for k, hit in census(found).items() if hit is True}
        cases += mine
    return cases


def build_multi():
    """Two and three codeblocks per TB, one layer, Qm 1, 2 and 6, symbols per layer no multiple of the codeblock count:
    the codeblocks differ in E, some E are no multiple of 32 and neighbours share an output word. rv 0 with the full
    buffer and rv 3 with a limited one, at a code rate of about one half and, for every second TB, with a selection
    that wraps."""
    cases = []
    for i, (nb, bg, C, Z) in enumerate(MULTI):
        for vi, (rv, kind) in enumerate(((0, "full"), (3, "lbrm_two_thirds"))):
            qm = (1, 2, 6)[(i + vi) % 3]
            bits = nb * 8 * (2 if (i + vi) % 2 == 0 else 9)
            nsym = bits // qm // C * C + 1 + (i % (C - 1) if C > 2 else 0)
            cases.append(dict(bg=bg, Z=Z, tb_index=0, tb_bytes=nb, rv=rv, kind=kind, role="multi_cb", qm=qm, layers=1,
                              nsym=nsym, Nref=nref_of(kind, bg, Z), codeblocks=C))
    return cases


def key(case):
    """What names a case in an assertion message."""
    return tuple(case[k] for k in ("bg", "Z", "tb_bytes", "rv", "kind", "role", "qm", "nsym", "Nref"))


def expected(orc, case):
    """The oracle's codeword (one bit per byte) of a case: chain_lib's composition."""
    from chain_lib import oracle_pdsch_encode
    cw, _, _ = oracle_pdsch_encode(orc, transport_block(case), case["bg"], case["rv"], case["qm"], case["layers"],
                                   case["Nref"], case["nsym"])
    return cw


def key_numbers(case):
    """A case's row in the golden file: bg, Z, TB bytes, rv, Qm, symbols, Nref and codeword bits."""
    return [case[k] for k in ("bg", "Z", "tb_bytes", "rv", "qm", "nsym", "Nref")] + [case["nsym"] * case["qm"]]


_CACHE = {}


def grid_with_expected(orc):
    """(cases, oracle codewords) of the grid, built once per process."""
    if "grid" not in _CACHE:
        cases = build_grid()
        _CACHE["grid"] = cases, [expected(orc, c) for c in cases]
    return _CACHE["grid"]


def multi_with_expected(orc):
    if "multi" not in _CACHE:
        cases = build_multi()
        _CACHE["multi"] = cases, [expected(orc, c) for c in cases]
    return _CACHE["multi"]


def golden_subset(cases):
    """Indices of the grid's cases at the lifting sizes of GOLDEN_Z."""
    return [i for i, c in enumerate(cases) if c["Z"] in GOLDEN_Z[c["bg"]]]
