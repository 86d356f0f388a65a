"""Random sequences of API calls against the oracle (tests/op_sequences.py has the model and the op table).  A
sampler carries lazy state of six kinds -- the terms table, the potential cache, deferred draws, plan levels and
their layouts, the trace ring, the Rao-Blackwell switch -- and every entry point of dwx_api.cc has to invalidate,
flush or snapshot the right part of it.  The other test files pin that along hand-picked lines; here the oracle is
stepped beside the sampler through 25 to 30 calls drawn at random, and the sampler's state is read only where the
sequence says so.  The sequences are committed as literal strings (TABLE); `generate` is the seeded generator
that drew them, kept so that the table can be extended -- the tests run the table, never a fresh draw.  Every
(graph, sequence) pair is one test: all of them on the emulated kernels (tests/hipemu), the first GPU_SEQUENCES of
every graph on the GPU.  test_coverage asserts, from the library's own counters, that the table still reaches the
states it is there for."""
import os
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import op_sequences as ops  # noqa: E402

GPU_SEQUENCES = 6
# graphs whose dwx_graph_info.grad_shift allows the packed collective (all-boolean, all-unary)
PACK_GRAPHS = ("small", "small_mixed", "small_sample_evidence", "small_learn_non_evidence", "small_plan_layouts")

# ------------------------------------------------------------------------ the generator
# one motif per sequence, by its index: the states the coverage test asks for do not depend on luck
MOTIFS = [
    "L R:f",              # a free-chain read flushes
    "L Xf",               # ... set_assignments
    "L W9",               # ... set_sweep
    "L H3",               # ... a halo exchange
    "L L D L",            # ... the free chain's pointer handed out; nothing defers from there
    "I S L F1S R:f",      # new weights between an inference sweep and the learning sweep that would read its cache;
                          # ... and between an un-split sweep's accumulation and its update, while its draws are owed
    "I I I",              # the terms table
    "T3 N5 T5 N2",        # one launch of more sweeps than the ring holds, one of fewer
    "L F2",               # a split sweep in pieces while draws are owed
    "L 2 L 2 I 2 I",      # both samplers of a pair advance while the other owes draws
    "I B3 L",             # the replica driver's averaging
    "P1 N3 R:b",          # Rao-Blackwell sums of a launch of several sweeps
]
WEIGHTED = [("L", 6), ("I", 5), ("F", 3), ("N", 2), ("S", 1), ("A", 1), ("B", 1), ("X", 2), ("H", 2), ("C", 1), ("W", 1),
            ("T", 2), ("P", 2), ("R", 3), ("2", 2)]


def generate(name, idx):
    """sequence `idx` of graph `name`: 25 to 30 ops, the motif of its index at a random place"""
    rng = np.random.default_rng([zlib.crc32(name.encode()), idx])
    pair = ops.graph_case(name)["pair"]
    kinds = [k for k, _ in WEIGHTED if pair or k != "2"]
    p = np.array([w for k, w in WEIGHTED if pair or k != "2"], float)
    motif = [t for t in MOTIFS[idx % len(MOTIFS)].split() if pair or t != "2"]
    n = int(rng.integers(25, 31)) - len(motif)
    out = []
    for _ in range(n):
        k = str(rng.choice(kinds, p=p / p.sum()))
        if k == "F":
            k += str(int(rng.choice([1, 2, 4]))) + ("G" if name in PACK_GRAPHS and rng.random() < 0.5 else "")
        elif k == "N":
            k += str(int(rng.integers(2, 6)))
        elif k in "AB":
            k += str(int(rng.integers(2, 4)))
        elif k == "X":
            k += "fe"[int(rng.integers(0, 2))]
        elif k == "H":
            k += str(int(rng.integers(1, 4)))
        elif k == "W":
            k += str(int(rng.integers(0, 1000)))
        elif k == "T":
            k += str(int(rng.choice([0, 2, 3, 4, 5, 5])))
        elif k == "P":
            k += str(int(rng.integers(0, 2)))
        elif k == "R":
            pick = [c for c in ops.ALL_OBSERVERS if rng.random() < 0.35]
            k = "R:" + ("".join(pick) or "w")
        out.append(k)
    at = int(rng.integers(0, len(out) + 1))
    return " ".join(out[:at] + motif + out[at:])


# ------------------------------------------------------------------------ the committed sequences
TABLE = {
    "small": [
        "R:fetw H1 L R:f S L T4 R:e I F1 R:etr T5 R:w R:fws W928 F2G F1G F1G Xe 2 I L I A2 L 2 N4 T0 L C",
        "T3 F2G F2 H3 Xe F2G I Xe I R:tb L F1G R:wz R:z T3 L Xf C L Xf W840 P0 R:fts L L L R:ws I L",
        "W46 P1 N5 I I N2 F1G L L L T2 S R:ewsz I L P1 Xe I T5 L W9 2 H1 R:frs C R:rb W818",
        "I F4G L 2 P1 H1 L I T0 B2 2 I P0 N2 L I R:t F2G T0 L I P0 I I L H3 I",
        "I L C I B3 C A2 I B2 L L D L B3 I F1 I I L Xe T5 N2 W752 R:twbs S L R:t N4 T5",
        "L L T2 S T5 I H2 I L B2 L H1 R:tr F2 R:ftbsz L C N4 L Xe L I S L F1S R:f 2 R:twsz",
        "L F1 I T4 L F2 H1 H1 S B3 2 C Xe T3 I I I L I L F4 N5 F2 I L C",
        "I C H3 I Xe L T3 N5 T5 N2 L F1 L Xf I I I I L F2G W57 T5 L B2 R:w",
        "L I I 2 L H1 2 B2 I W48 N3 B3 2 I W993 L I I I 2 F1 F4G L I 2 I L F2 L F2",
        "I P1 L L Xe A2 P0 L T5 L L F2 L W398 L 2 L 2 I 2 I L L H1 R:trz",
        "R:ewb F4 H1 L I T4 W194 S A3 2 R:z H3 I B3 L I Xe I F4 H3 N2 L N2 A2 L 2 I",
        "R:er 2 I N2 F2 T2 L Xe T5 B2 I L T5 I L I P1 N3 R:b T5 I N4 L L L P1 Xe R:fsz I I",
    ],
    "small_mixed": [
        "R:trs L R:f A2 I I P1 2 R:erz A2 H1 R:ferbs 2 H2 W775 H2 L 2 P1 T4 I W676 L R:eb R:fs C I",
        "P1 Xe I Xe L N3 R:ewb 2 N4 N5 R:trs L L S Xe R:w C N2 R:fwbz A2 I L Xf 2 L I S",
        "I F2 L T5 I S T3 2 L F2G I A2 L S C 2 I N3 H3 I L L W9 F1G B2 H2",
        "I 2 2 Xe W992 L F4 2 L C L N4 L H3 I L L L F4 R:wbz W993 R:ebs 2 A3 T3 I F1G",
        "L P1 L Xe T3 N3 S I L L I N3 Xf B3 T3 F4 L L D L I F1G H2 L R:etr",
        "I I T4 C B3 R:w L T2 I S L F1S R:f B3 A2 I L I I F2 P1 F2G H1 L I F1 2 L R:ferz",
        "S I I L H1 S I T4 L H1 2 I I I I C P0 F1 I I I R:wrz I H3 P0 L H1",
        "T3 H1 I T3 N5 T5 N2 H2 A2 R:b P0 I I R:ftb I N5 L A2 F1 P1 L H2 I P1 A3 F2 I F4G N2",
        "2 P0 W894 P1 F1 I I B3 Xf B2 L I L F2 T5 F4 P0 I H3 I F2 R:e C I I 2 L",
        "F1G B2 L I A3 L C L 2 L 2 I 2 I L P1 L R:etwrb R:fz N4 L R:ftwrs F2 Xe P0 P0 N2 F1G P1 H3",
        "N3 L S L F2 2 A2 N5 L L A2 R:erb L P1 C L 2 I F2G I B3 L L 2 C 2 H3 F2G 2 Xe",
        "F2 N5 R:trb L N4 I H1 F1 R:fetbz 2 P1 N3 R:b W828 A3 I L C H2 I B3 F1 F2 L L",
    ],
    "small_sample_evidence": [
        "N2 P1 L T2 R:fb F1 W48 Xe L P0 T5 P1 N2 L N4 L R:f Xe I L R:rbs C T5 L F1 L L Xf H1 H2",
        "L P1 I I I Xf F4G R:etb T2 F1G I L Xf Xf N5 I H1 N4 C I B3 I N3 B2 B3 F1",
        "F4 N5 R:fetwsz R:fw I Xe P1 S T0 C R:ew R:fetsz L W9 L I T0 C R:etwrb R:fesz R:ftwr H3 F2G Xf I R:ez I",
        "L H1 L H3 T3 F4G F2 F1G F1G A3 H3 P0 R:ws B3 R:fbz L A2 F1G T4 Xe I R:er F1 I P0 F4G A2 I H3",
        "I B3 F4G I I Xe Xe I F4G L L D L I F2 H2 I R:et N2 H2 A2 Xe W446 I S I N3 F1G F2 C",
        "F4 F1 H2 T2 I N2 L R:wsz I L W374 L A3 I S L F1S R:f T5 L H2 R:feb N3 P1 I R:wb I R:tb P1",
        "I I R:fez I L F4 I H1 B3 F1 I I I N5 L I R:fr I Xe L L I H2 L I I B3 C H3 I",
        "I R:ftw I L R:fwb L R:ewbz N5 T3 R:twb P0 I N5 L N2 I R:fetwr L T3 N5 T5 N2 L P1 Xf",
        "A2 I T0 L N3 L F4 I L L L L F4G T0 L N2 L F2 I S L P0 N5 P1 S",
        "T0 C L A2 L I L I T3 Xe I L L I I L L R:ws H1 L Xf I P1 I L",
        "R:tw R:w W302 I I H1 B3 F2G N3 I I L L L L N5 L A3 I B3 L I L R:fetbs I L",
        "I P1 N3 R:b I I C L H2 I L F2 L F4 I S F4G I H3 R:b Xf L N4 L R:fe T0 L",
    ],
    "small_learn_non_evidence": [
        "N5 R:wrb Xe T0 L R:fw I L T2 F2 A3 L R:f T4 T4 Xf I L L A2 R:wrz Xf T0 N2 R:z L L P0 I",
        "R:rz C I Xe I L L Xf R:wrbz B3 L I L R:ewr I P1 L R:bs L B2 Xf W171 L B3 L L I P1",
        "B3 C L A3 Xe A2 L I R:fetwrz R:w A2 H2 L R:s N4 N3 R:t I R:wbs B3 F1G R:ftbsz C L B2 I L W9 Xe",
        "Xf B3 N2 F1 F4 F4 I L I I W659 N3 L H3 I H1 T3 B3 N4 N2 F4 F4 I C L I",
        "Xf W496 T5 S L R:e C L L D L W504 L P0 S P0 H3 F1G P0 P1 F2G I L R:fer F2 F1G N5 I R:frbs",
        "N2 I N3 H3 T4 W674 I S L F1S R:f T3 I I L T3 F2G R:tz R:fersz P1 Xf C H2 F2G R:r",
        "N4 R:e L L R:ws H1 Xf L C F2 R:f N3 L T5 P0 I F2 T4 F2G I I I I P1 L L H2 A3 Xe",
        "L B2 H2 P1 Xf R:s C T4 I H3 L T3 N5 T5 N2 L L P0 S B3 F4G H2 L S T4",
        "I I R:ftb L F1G R:ewb I N2 I I A2 L P1 I I T5 W893 I F4G I P0 L R:fs L F2 L I I",
        "S F4 P1 N4 R:es B2 W738 Xe A3 P0 W901 L H2 L L L I I I L F2 N5 L T5 I",
        "N4 I P0 R:rsz P0 I B3 L P0 N2 Xe N4 R:trb T4 I N2 I I I R:twrbz I R:w F4 N3 N2 B2",
        "R:fwrz S I I I H2 C L I R:s L Xf R:tbs P1 N3 R:b I S S L L F1G R:twsz H2 R:etrs T2 F4",
    ],
    "small_plan_layouts": [
        "R:ftwbz L L R:ferb R:fbz P0 W119 W500 C H2 H2 R:eb P0 A2 L R:f L H1 P1 L L N2 P1 B2 I I L",
        "N2 I L Xf I R:tz H2 F4G I R:etbz L L I H2 F4G L F2 T5 S Xf Xe N3 I F2G F2G N4 Xe W529 L",
        "L L R:etrz L I I F1G L N3 C F1 L W9 C R:ersz I T5 L R:ftwrz I T4 L L L I",
        "C N3 A2 I F1 I L H3 I T2 I L I I L A2 R:erb L I I Xf R:w R:frbs I L S P1",
        "P1 I Xf L W308 Xf L L N5 T5 P1 W765 T5 F4G L H1 H1 L Xf H1 F4G L L D L P0 F2G",
        "R:fetwr B2 L I I F1G Xe I S L F1S R:f L Xe N2 T5 H3 A2 L R:fewbz I T0 L L W275 T4",
        "R:fr T0 P1 F2G Xf B3 T0 A2 F4 F2 N3 A2 H2 W506 A3 Xf I I I I R:etrb C N2 C P1 T4 I H3 P0",
        "I H3 B2 I F2 H2 L I C A2 F2G L F2 N2 F2G R:ewz Xe Xe L I I L F2 T3 P0 L T3 N5 T5 N2",
        "B2 I T5 Xf L C N4 S I H2 P0 L F2 T5 F4 L I R:es P1 R:er W316 T2 A2 L Xe N2 S I T5",
        "T5 R:er I I R:wrbsz T3 L L H2 Xe R:etwr W640 S R:fetz L L L I I P0 I P0 N3 F2 F1 L P0 H1",
        "Xe F2 N4 Xe A2 R:wz B3 I L R:fbs I T4 R:trs I F1G W935 L I I H2 W785 I B3 L L S H1",
        "R:fets Xf R:twbz P1 N3 R:b W108 H1 R:ft L Xe Xe L H3 R:rbs N2 L Xf I H2 R:t R:twrbs Xe Xe L I H1 C L",
    ],
    "cfg3b": [
        "F4 Xe L L R:f T3 I C L P1 N3 H3 R:trbz B2 L B2 R:fetbz N4 R:erb L Xe I F1 R:twbz L S B2",
        "P0 I L P0 F1 2 R:ewz B3 C T3 H3 I W889 H3 R:s L Xf I I R:etb H3 I B3 W844 L I L I W521 L",
        "L W9 Xe T5 S S T0 N5 P0 L I I T5 L H1 R:fetwrb L T5 W878 I B3 H1 A3 2 C",
        "R:wrbsz L I N5 I P0 B3 L L H3 A2 H3 I C L F2 T0 B3 L L W862 N3 I F4 I L H3 Xe L L",
        "H1 F2 2 W694 T2 P1 L H3 N2 N4 F4 L R:fers 2 R:rs Xe L L D L Xf A3 A3 Xe F4 W457 S S F2",
        "L T4 I S B2 I F4 H3 C S I H3 B3 I I L I L I I I S L F1S R:f I R:bz L I I",
        "I I I I A3 N3 F2 T3 I C S 2 I I R:frbsz L L C R:twb Xf T4 N4 R:fersz L C L H2 H2",
        "2 C F2 L F4 Xe A3 I F4 I F4 C H3 S L I N3 I L L T2 L T3 N5 T5 N2 P1 B3",
        "L L F2 L I R:b R:frbz Xe N5 2 S L L R:ewrz T0 L F2 N3 I R:etz W655 L Xf S T5 L 2",
        "H1 L H3 F2 H2 P0 F4 I F4 L L R:wr I I L L 2 L 2 I 2 I 2 P0 T4 B2 T4 L",
        "2 I I L 2 L L Xf Xe L I N2 L N5 B3 I I I A3 2 A3 I I B3 L C T5",
        "S R:etrs F1 L L S T3 C L I B2 T5 H3 L I F4 N4 L R:fewz I R:wb P1 N3 R:b T5 T3 I S 2",
    ],
    "cfg4b": [
        "L I C Xf I W993 I F2 L H3 A2 T5 I F4 C H3 I P0 S S L R:f T3 L H2 F1 L",
        "Xf P0 Xe T0 A3 P1 L R:ftrbz I H3 B3 W649 L T3 L H1 Xf I L Xf L Xe F2 I W740",
        "R:wrs R:ers F4 F4 L I Xf Xf T5 L W9 B2 L Xe L L L P1 L R:fz Xf L B2 W738 N5 H1 L L",
        "Xe L B2 L Xe L H2 C N4 I R:w Xf B2 Xf I C L I L L H3 L L L Xe R:ewrbz",
        "R:frb P1 F1 N2 H3 L L D L A2 L F1 Xe C F1 L T3 N3 L I L A2 F2 Xf F1 T3 L",
        "Xe R:etws P0 I S H2 P0 H3 L T5 I R:ebs R:fwb I S L F1S R:f W160 N2 C L F2 I H3 L",
        "F4 T5 C I I I I S C I F2 R:ewbs I L S H2 I R:w B3 L N2 P0 L T0 H1 B2",
        "Xf P1 L A3 R:ebz L A2 C P0 P0 N5 F4 H2 H2 T5 T0 L R:erbs N2 F1 B3 T3 N5 T5 N2 S L",
        "L S L F2 C I L R:es F2 A3 C T0 C L L F2 P0 N3 H3 R:ftb H2 L P1 A3 R:ftwb I L L",
        "R:bs L L I I I L C I R:rb H1 F4 W607 C T5 H3 L C C T5 F4 Xe I I L T5 I",
        "I B3 L I N5 H1 I P1 L R:er I H1 P0 I L L N2 Xe R:fer T3 I F1 L Xe Xe L N3 L",
        "P1 T5 L N5 B2 L N5 H3 I I R:tz L P1 N3 R:b Xf P0 F4 F1 F4 N2 L H1 H2 L F4 I Xe",
    ],
    "random": [
        "L P1 I I I W752 L F2 F1 F2 B3 L L B2 R:trs R:erz A2 C F2 L L R:f Xe C I",
        "P0 L R:ewrz F2 A2 F2 C Xe L Xf C L L F1 C A2 L A2 I P1 L Xf Xe H3 Xe",
        "I H1 N3 I L L L L L L L B3 L R:ewb C A3 L W9 Xf F2 L I F1 Xf F2",
        "L H3 I H3 Xf L P0 R:febs L L L Xe L I L I W58 Xf L Xe I F4 P0 I L",
        "L N4 I C I L R:etwrz H2 I L F1 I I P0 L F2 A2 B2 L L D L L H1 I F4 R:fwz T3",
        "T5 N4 L B3 H3 Xe P1 P1 F1 I I S L F1S R:f L L C I H2 P0 L I T4 W888",
        "C L P0 Xe N4 L P1 N5 I P0 L H2 H2 F4 N3 I I I L L C T0 I I N2 L T4",
        "S L T3 F4 W212 P1 T3 N5 T5 N2 I L S Xf R:rbs P1 I Xf L L I I Xf A3 Xf",
        "T5 R:tsz F4 F4 P1 R:ftsz I I R:fetb I H2 W302 I Xe L L L L F2 N5 C R:fb Xe N5 F1 H1 H2 P0",
        "A2 H1 I Xf Xf I R:ferbs T5 H2 P1 I P1 F2 T5 N4 L L I I R:ftwb L F2 N5 H1 R:w F1",
        "H1 H3 I P1 N4 L L L F2 R:frb H1 B3 W979 L F4 I I B3 L S I P1 L F2 B3 S W306 P0 H3",
        "L I R:wbs I I L I H2 I L Xe P0 Xf Xe R:tbs R:tsz L Xf P1 N3 R:b I I F1 H1 P0 I I P0",
    ],
    "ghost": [
        "L I I P1 I F1 N4 N3 Xf I L Xf B2 H2 I I L L Xf F4 A2 L W288 C H2 L R:f A2",
        "N4 L Xf P0 F4 F4 F2 A3 I F1 L I L I I P1 R:fbs N5 L I F1 Xe P0 L Xf T4 F1 L",
        "T3 P0 F2 L L W9 F1 F2 P1 R:fb I F1 L A3 L I I R:ft I P0 F2 I Xe I N3 I S P1 I",
        "R:r P1 L I Xe L L H3 I L F4 N4 W828 P0 T5 L L R:twbs I T4 H2 P1 H3 Xf C I L I L L",
        "Xf Xe I N2 N3 L I S T3 A3 I P1 I P1 W286 L H2 L N3 B2 I R:w T0 L L D L L L B2",
        "L S I I S L F1S R:f P0 P0 A2 L T3 B3 I R:e N4 Xf A3 L I L H3 L W752 Xe C I I C",
        "L W999 I I I I I I I L T5 L N4 I A3 R:ez A2 T5 Xf L F4 L R:wbz N2 Xe",
        "I T0 H2 I L L N4 P1 C L N4 N2 F2 T3 N5 T5 N2 R:es L N3 T4 L F2 T5 T5 W378 P1 I",
        "R:es L N4 L B2 T2 L H2 I R:ftwrb L N5 I R:fewbs L I I W849 L Xf H1 C L F2 R:ebs",
        "L F1 H3 P1 I W151 T4 L L A2 L F4 I P1 I L C L Xe Xf W366 F4 I P0 L L I I",
        "F2 P1 I N3 L S N5 R:erb B2 P1 I L I Xf A2 I B3 L F4 T3 T2 T3 Xe I P0",
        "I H3 I I N2 W76 L Xe Xf L Xf F2 S S I S P1 N3 R:b L Xe F1 P0 P0 P0",
    ],
    "few_weights": [
        "S N4 2 2 L L L R:fetrs Xe F2 I N5 C L 2 R:wr Xf R:eb R:wrbs R:wb L R:f P1 L 2 N2 R:ftr",
        "F1 N3 L L L A3 P0 L L I Xf B3 L Xf L N2 L N3 P0 R:fw L I Xe R:ftw H2 R:frz N5",
        "I Xf L L W382 B2 T2 F1 2 L F4 A2 I A3 Xe R:wbs Xe L L Xf I L W9 C H3 T3",
        "W125 L T0 Xf 2 I W394 L H3 Xe F4 I T4 2 F1 L Xf P0 I N3 2 I P1 L S I I L R:twsz",
        "Xe F2 Xe L 2 F1 T5 T3 I S T5 R:tsz L L D L I L 2 C S N3 S I L L H1",
        "L H3 F2 T5 N3 F1 F4 W719 T0 L F4 B2 I S L F1S R:f T2 Xf 2 L H1 N4 L N4 T2 F2 I",
        "I Xf H2 N5 F4 H1 W1 2 2 P1 P0 I I I 2 I C L I R:e F4 2 S S L L P1",
        "L T3 F4 R:e I B2 F4 C C A2 I I N2 L L N5 T3 N5 T5 N2 W107 P1 L F2 L Xe R:wrz",
        "T0 H3 T3 R:twb R:fts F2 I P0 I L L N2 Xe R:wrbsz W389 P1 T0 Xe W492 I L F2 L N4 L A3 W585 L",
        "P1 L P1 L N5 Xf F1 R:ftbz L 2 L F4 N3 L I N2 L L 2 L 2 I 2 I F1 A2",
        "H2 Xe I N3 H2 L P0 L A2 I L N4 N2 F1 H3 I F1 H3 I I B3 L A3 L R:fewrs L Xf W96",
        "I L R:fs P0 2 C F2 Xe P1 N3 R:b 2 H2 N4 L I L P1 H2 H3 L F4 L I I R:w C I L T3",
    ],
}


# ------------------------------------------------------------------------ running them
_emu = []
COVERAGE = {}       # (graph, index) -> (Model.cov, Model.counters()) of the emulated run


def _library(where):
    from parity import emu_library, gpu_library
    if where == "gpu":
        return gpu_library()
    if not _emu:
        _emu.append(emu_library())
    return _emu[0]


@pytest.fixture(autouse=True)
def sorted_small(monkeypatch):
    # (the weight-sorted copy engages from 4096 weights on its own)
    monkeypatch.setenv("DWX_SORTED_MIN_W", "0")


def _run(where, name, idx):
    m = ops.Model(_library(where), name, rng_seed=idx).run(TABLE[name][idx])
    if where == "emu":
        COVERAGE[(name, idx)] = (m.cov, m.counters())
    return m


CASES = [pytest.param("emu", name, i, id="emu-%s-s%02d" % (name, i)) for name in TABLE for i in range(len(TABLE[name]))]
CASES += [pytest.param("gpu", name, i, id="gpu-%s-s%02d" % (name, i), marks=pytest.mark.gpu)
          for name in TABLE for i in range(min(GPU_SEQUENCES, len(TABLE[name])))]


@pytest.mark.parametrize("where,name,idx", CASES)
def test_sequence(where, name, idx):
    _run(where, name, idx)


def test_table_shape():
    assert set(TABLE) == set(ops.GRAPHS)
    for name, seqs in TABLE.items():
        assert len(seqs) >= 12 and len(set(seqs)) == len(seqs), name
        for text in seqs:
            parsed = ops.parse(text)
            assert 25 <= len(parsed) <= 30, (name, text)
            assert " ".join(ops._token(op) for op in parsed) == text
            if name not in PACK_GRAPHS:
                assert not any(op[0] == "F" and op[2] for op in parsed), (name, text)
            if not ops.graph_case(name)["pair"]:
                assert ("2",) not in parsed, (name, text)


def test_coverage():
    """the table cannot go hollow: the states it is there for are reached, by the library's own counters (emulated)"""
    for name in TABLE:
        for idx in range(len(TABLE[name])):
            if (name, idx) not in COVERAGE:       # (run on its own, or that sequence was deselected)
                _run("emu", name, idx)
    per_graph = {}
    for (name, idx), (cov, cnt) in COVERAGE.items():
        g = per_graph.setdefault(name, dict(flush_by=set(), deferred=0, flushes=0, pot_cache=0, merged=0))
        g["flush_by"] |= cov["flush_by"]
        g["deferred"] += sum(cnt["deferred"]); g["flushes"] += sum(cnt["flushes"])
        g["pot_cache"] += cnt["pot_cache"]; g["merged"] += cnt["merged"]
        for k in ("i_then_weights_then_l", "three_i", "n_cap_below", "n_cap_above", "split_f_owed", "pair_advance_owed"):
            g[k] = g.get(k, False) or cov[k]
    eligible = [name for name in TABLE if ops.graph_case(name)["defer"]]
    assert len(eligible) >= 4
    for name in eligible:
        g = per_graph[name]
        assert g["deferred"] > 0 and g["flushes"] > 0, (name, g)
        assert g["flush_by"] >= {"free_read", "X", "W", "H", "D"}, (name, g["flush_by"])       # every trigger of a flush
        assert g["pot_cache"] > 0, (name, g)
        assert g["split_f_owed"], name
    for name in TABLE:
        g = per_graph[name]
        assert g["i_then_weights_then_l"] and g["three_i"] and g["n_cap_below"] and g["n_cap_above"], (name, g)
        if not ops.graph_case(name)["defer"] and name != "few_weights":
            assert g["deferred"] == 0 and g["flushes"] == 0, (name, g)          # (and the others never defer)
        if ops.graph_case(name)["pair"] and ops.graph_case(name)["defer"]:
            assert g["pair_advance_owed"], name
    assert any(ops.graph_case(name)["pair"] and ops.graph_case(name)["defer"] for name in TABLE)
    assert per_graph["few_weights"]["merged"] > 0, per_graph["few_weights"]


if __name__ == "__main__":
    # python tests/test_op_sequences.py [N]: a fresh table of N (default 12) sequences per graph, to paste above
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 12
    print("TABLE = {")
    for name in ops.GRAPHS:
        print('    "%s": [' % name)
        for i in range(n):
            print('        "%s",' % generate(name, i))
        print("    ],")
    print("}")
