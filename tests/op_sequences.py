"""The model behind tests/test_op_sequences.py: one dwx.Graph, one or two GibbsSamplers on it (different seeds) and
one oracle per sampler, stepped side by side through a sequence of API calls.  Every op is applied to the sampler
and mirrored on the oracle; NOTHING of the sampler's state is read except where the sequence says so (an R op), so
that learning sweeps really run deferred, the potential cache and the terms table really stay live, and every entry
point of dwx_api.cc has to invalidate, flush or snapshot the right part of that lazy state on its own.

A sequence is a string of tokens:
  L        sample_sgd                          F<b>[G][S]  the sweep in pieces under sgd_plan(step, b): accumulate,
  I        sample()                                     apply per chunk as parity.learn_sweep_both mirrors it; G: grad_pack
  N<k>     sample_n(k)                                  + grad_unpack before every apply (an identity on DWX_BUF_GRAD);
                                                        S: new weights through the setter before the first apply
  S        new weights through the setter      A<n>     average_weights(n)
  B<n>     n x the weights written into DWX_BUF_WEIGHTS with dwx_buffer_copy, then average_weights(n)
  X<f|e>   set_assignments of a chain, about 50 values changed (the evidence chain: query variables only)
  H<mask>  halo pack(mask) -- the buffer must hold the oracle's values -- then new values written into the buffer
           and unpack(mask); a list over a third of the owned variables (and one over the ghosts where there are any)
  C        clear_tallies (empties the trace and the Rao-Blackwell sums too: include/dwx.h at dwx_rb_enable and
           dwx_trace_enable)
  W<n>     sweep = n                           T<cap>   trace_enable(cap)         P<0|1>  rb_enable
  D        device_buffer(BUF_ASSIGN_FREE): from there no learning sweep of that sampler defers
  2        the following ops address the other sampler of the pair
  R:<set>  read and compare: f free chain, e evidence chain, t tallies and nsamples, w weights, r the trace
           (ids, planes, co-occurrence counts, diagnostics), b rb_sums, s score(free), z score(evid)
Every sequence ends with all observers.  The counters the coverage test needs are taken from the library
(dwx_kernel_time) around every op."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import binding as orc  # noqa: E402
from sampler_amd import diagnostics, dwx, synthetic  # noqa: E402
from parity import learn_sweep_both  # noqa: E402

WTOL = 1e-12            # run_parity's tolerance on the weights
SEEDS = (77, 1077)
STEP, DECAY = 0.01, 0.9
ALL_OBSERVERS = "fetwrbsz"
RB_PICK = 40            # variables per launch whose Rao-Blackwell rows meet the oracle


# ------------------------------------------------------------------------ the graphs
def _small():
    from test_pot_cache import make_graph
    return make_graph("small")


def _graph_small():
    raw, copts, _ = _small()
    return dict(raw=raw, copts=copts, pair=True, defer=True)


def _graph_small_mixed():
    from test_pot_cache import make_graph
    raw, copts, _ = make_graph("small_mixed")
    return dict(raw=raw, copts=copts, pair=True, defer=True)


def _graph_small_se():
    raw, copts, _ = _small()
    return dict(raw=raw, copts=copts, kw=dict(sample_evidence=True), defer=True)


def _graph_small_lne():
    raw, copts, _ = _small()
    return dict(raw=raw, copts=copts, kw=dict(learn_non_evidence=True))


def _graph_small_layout():
    raw, copts, _ = _small()
    return dict(raw=raw, copts=copts, kw=dict(plan_layouts=1), defer=True)


def _graph_cfg3b():
    return dict(raw=synthetic.cfg3b(3000, n_weights=500), pair=True)


def _graph_cfg4b():
    return dict(raw=synthetic.cfg4b(600, card=5, n_weights=60))


def _graph_random():
    from randgraph import random_graph
    # (RATIO at arity 3 takes log2(3) on the device: no exact score, the graph is compiled without its factor table)
    return dict(raw=random_graph(44, V=600, F=3000, W=30, p_cat=0.6, max_arity=3, exact_fvals=True),
                copts=dict(tile_vars=64), kw=dict(noise_aware=True), score=False)


def _graph_ghost():
    from sampler_amd.shard import make_shard
    local, _ = make_shard(synthetic.cfg3b(600, n_weights=24, seed=21), 150, 420)
    assert local.num_ghost_variables > 0
    return dict(raw=local)


def _graph_few_weights():
    # 8 weights tied to 1500 evidence factors each: at step_cap 0.05 the learning sweeps split, one launch per mini-batch
    return dict(raw=synthetic.cfg4(3000, card=8, seed=7, learn=True), step_cap=0.05, pair=True, merged=True)


GRAPHS = {
    "small": _graph_small, "small_mixed": _graph_small_mixed, "small_sample_evidence": _graph_small_se,
    "small_learn_non_evidence": _graph_small_lne, "small_plan_layouts": _graph_small_layout, "cfg3b": _graph_cfg3b,
    "cfg4b": _graph_cfg4b, "random": _graph_random, "ghost": _graph_ghost, "few_weights": _graph_few_weights,
}
_built = {}


def graph_case(name):
    """the named graph's description, built once: raw graph, compile and sampler options, the score expectation"""
    case = _built.get(name)
    if case is None:
        case = dict(copts={}, kw={}, pair=False, defer=False, merged=False, score=True, step_cap=1.0)
        case.update(GRAPHS[name]())
        assert case["raw"].num_variables <= 4100
        case["expect"] = None
        if case["score"]:
            from test_score import Expect
            case["expect"] = Expect(case["raw"])
        _built[name] = case
    return case


# ------------------------------------------------------------------------ tokens
def parse(text):
    ops = []
    for tok in text.split():
        k = tok[0]
        if k in "LISCD2" and len(tok) == 1:
            ops.append((k,))
        elif k == "F":
            digits = tok[1:].rstrip("GS")
            tail = tok[1 + len(digits):]
            if tail not in ("", "G", "S", "GS"):
                raise ValueError("unknown op %r" % tok)
            ops.append(("F", int(digits), "G" in tail, "S" in tail))
        elif k in "NABHWTP":
            ops.append((k, int(tok[1:])))
        elif k == "X" and tok[1:] in ("f", "e"):
            ops.append(("X", tok[1:]))
        elif tok.startswith("R:") and len(tok) > 2 and set(tok[2:]) <= set(ALL_OBSERVERS):
            ops.append(("R", tok[2:]))
        else:
            raise ValueError("unknown op %r" % tok)
    return ops


class SequenceFailure(AssertionError):
    pass


class Side:
    """one sampler, its oracle and what the model remembers for it"""

    def __init__(self, model, seed):
        case, g = model.case, model.g
        raw = case["raw"]
        self.seed = seed
        self.o = orc.Oracle(raw, **{k: v for k, v in case["kw"].items() if k != "plan_layouts"})
        self.o.set_fixed_point_mask(g.fixed_point_mask())
        self.s = dwx.GibbsSampler(g, seed=seed, step_cap=case["step_cap"], **case["kw"])
        self.sweep, self.cur = 0, STEP
        # the trace as include/dwx.h describes it: a ring of (sweep id, the owned variables' evidence-chain values)
        self.trace_ever, self.trace_on, self.trace_cap, self.ring = False, False, 0, []
        # the Rao-Blackwell sums of the picked variables, accumulated as tests/test_rao_blackwell._against_oracle does
        self.rb_ever, self.rb_on, self.rb_n = False, False, 0
        self.rb_expected = np.zeros(self.o.num_values)
        self.handed_out = None          # the deferred-sweeps counter when D handed the free chain's pointer out
        self.owed = False               # the last learning sweep deferred and nothing has flushed since
        rng = np.random.default_rng(seed)
        n_owned = model.n_owned
        self.halos = [self._halo(np.sort(rng.choice(n_owned, n_owned // 3, replace=False)))]
        if model.n_owned < raw.num_variables:
            self.halos.append(self._halo(np.arange(model.n_owned, raw.num_variables)))
        sampled = model.sampled
        self.rb_pick, self.rb_checked = [], np.zeros(self.o.num_values, bool)
        for L in range(len(model.off) - 1):
            sl = model.order[int(model.off[L]):int(model.off[L + 1])].astype(np.int64)
            mine = sl[sampled[sl]]
            mine = np.sort(rng.choice(mine, min(RB_PICK, len(mine)), replace=False)) if len(mine) else mine
            self.rb_pick.append(mine.tolist())
            for v in mine.tolist():
                self.rb_checked[model.base[v]:model.base[v] + model.rows[v]] = True

    def _halo(self, vids):
        return dict(vids=np.asarray(vids, np.int64), h=dwx.HaloList(self.s, vids))

    def counters(self):
        _, flushes, deferred = self.s.kernel_time("deferred")
        return flushes, deferred


class Model:
    def __init__(self, lib, name, rng_seed=0):
        self.name, self.case = name, graph_case(name)
        case = self.case
        raw = self.raw = case["raw"]
        copts = dict(case["copts"])
        if case["score"]:
            copts["keep_factors"] = 1
        self.lib = lib
        self.g = dwx.Graph(raw, lib=lib, **copts)
        self.order, self.off = self.g.schedule()
        self.n_owned = raw.num_variables - raw.num_ghost_variables
        dtype = np.asarray(raw.var_dtype)
        self.card = np.where(dtype == 0, 2, np.asarray(raw.var_cardinality)).astype(np.int64)       # dense values [0, card)
        self.rows = np.where(dtype == 0, 1, np.asarray(raw.var_cardinality)).astype(np.int64)       # value rows
        self.base = np.asarray(self.g.values()[0], np.int64)
        self.role = np.asarray(raw.var_role)
        self.sampled = np.ones(raw.num_variables, bool) if case["kw"].get("sample_evidence") else self.role == 0
        self.sampled[self.n_owned:] = False
        self.sides = [Side(self, SEEDS[i]) for i in range(2 if case["pair"] else 1)]
        self.active = 0
        self.rng = np.random.default_rng([rng_seed, 5])
        self.log = []
        # what the coverage test asks for (tests/test_op_sequences.py)
        self.cov = dict(flush_by=set(), i_then_weights_then_l=False, three_i=False, n_cap_below=False, n_cap_above=False,
                        split_f_owed=False, pair_advance_owed=False)
        self._since_i = None       # ops since the last I: None, or whether the weights changed since
        self._i_run = 0            # consecutive inference sweeps of the active sampler without a weight change
        self._advanced_owed = set()    # the samplers that ran a sweep while the other one owed draws
        assert self.sides[0].o.sched_check_independent(self.order, self.off)

    # -------------------------------------------------------------------- running
    def run(self, text):
        ops = parse(text) + [("R", ALL_OBSERVERS)] + ([("2",), ("R", ALL_OBSERVERS)] if len(self.sides) > 1 else [])
        try:
            for op in ops:
                self.log.append(op)
                self.apply(op)
        except SequenceFailure:
            raise
        except Exception as e:       # an observer's assertion, a DwxError: the same report
            raise SequenceFailure(self.report("%s: %s" % (type(e).__name__, e))) from e
        return self

    def report(self, what):
        return "graph %s, after %s: %s" % (self.name, " ".join(_token(op) for op in self.log), what)

    def check(self, ok, what):
        if not ok:
            raise SequenceFailure(self.report(what))

    def counters(self):
        """from the library: per sampler (flushes, learning sweeps that deferred), pot-cache sweeps, merged sweeps"""
        return dict(flushes=[sd.counters()[0] for sd in self.sides], deferred=[sd.counters()[1] for sd in self.sides],
                    pot_cache=sum(sd.s.kernel_time("pot_cache")[2] for sd in self.sides),
                    merged=sum(sd.s.kernel_time("merged")[1] for sd in self.sides))

    # -------------------------------------------------------------------- ops
    def apply(self, op):
        sd = self.sides[self.active]
        k = op[0]
        f0, d0 = sd.counters()
        other_owed = any(x.owed for x in self.sides if x is not sd)
        if k == "L":
            batches = learn_sweep_both(sd.s, sd.o, self.order, sd.seed, sd.sweep, sd.cur)
            self._learned(sd, d0, batches)
        elif k == "F":
            batches = self._pieces(sd, op[1], op[2], op[3])
            self._learned(sd, d0, batches)
        elif k == "I":
            sd.s.sample(); sd.s.wait()
            self._oracle_sweeps(sd, 1)
        elif k == "N":
            if sd.trace_on and sd.trace_cap < op[1]:
                self.cov["n_cap_below"] = True
            if sd.trace_on and sd.trace_cap > op[1]:
                self.cov["n_cap_above"] = True
            sd.s.sample_n(op[1]); sd.s.wait()
            self._oracle_sweeps(sd, op[1])
        elif k == "S":
            w = sd.s.weights + self.rng.normal(0.0, 0.25, sd.s.W)
            sd.s.weights = w
            sd.o.weights[:] = w
        elif k == "A":
            sd.s.average_weights(op[1]); sd.s.wait()
            self._oracle_average(sd, np.array(sd.o.weights), op[1])
        elif k == "B":
            # the replica driver's way: the sum over n replicas lands in DWX_BUF_WEIGHTS behind the library's back
            summed = np.ascontiguousarray(op[1] * sd.s.weights)
            ptr, nbytes = sd.s.device_buffer(dwx.BUF_WEIGHTS)
            self.lib.check(self.lib.L.dwx_buffer_copy(sd.s.h, ptr, summed.ctypes.data, nbytes, 1))
            sd.s.average_weights(op[1]); sd.s.wait()
            self._oracle_average(sd, op[1] * np.array(sd.o.weights), op[1])
        elif k == "X":
            self._set_assignments(sd, op[1])
        elif k == "H":
            for halo in sd.halos:
                self._halo(sd, halo, op[1])
        elif k == "C":
            # include/dwx.h: "dwx_clear_tallies zeroes them with the tallies" (dwx_rb_enable) and "empties the trace
            # with the tallies" (dwx_trace_enable)
            sd.s.clear_tallies(); sd.o.clear_tallies()
            sd.ring = []
            sd.rb_expected[:] = 0.0
            sd.rb_n = 0
        elif k == "W":
            sd.s.sweep = op[1]
            sd.sweep = op[1]
        elif k == "T":
            sd.s.trace_enable(op[1])
            if op[1] == 0:
                sd.trace_on = False          # include/dwx.h: "capacity 0 stops recording and keeps what is there"
            else:
                if not sd.trace_ever or op[1] != sd.trace_cap:
                    sd.ring = []             # "a different non-zero capacity reallocates and empties the ring"
                sd.trace_ever, sd.trace_on, sd.trace_cap = True, True, op[1]
        elif k == "P":
            sd.s.rb_enable(bool(op[1]))
            sd.rb_on = bool(op[1])
            sd.rb_ever = sd.rb_ever or sd.rb_on
        elif k == "D":
            if sd.handed_out is None:
                ptr, nbytes = sd.s.device_buffer(dwx.BUF_ASSIGN_FREE)
                self.check(ptr and nbytes == 4 * self.raw.num_variables, "device_buffer(BUF_ASSIGN_FREE)")
                sd.handed_out = sd.counters()[1]
        elif k == "2":
            if len(self.sides) > 1:
                self.active = 1 - self.active
                self._since_i, self._i_run = None, 0
        elif k == "R":
            self._read(sd, op[1])
        else:
            raise ValueError(op)
        # ---- bookkeeping from the library's counters
        f1, d1 = sd.counters()
        if f1 > f0:
            sd.owed = False
            what = {"X": "X", "W": "W", "H": "H", "D": "D"}.get(k)
            if what:
                self.cov["flush_by"].add(what)
        if sd.handed_out is not None:
            self.check(d1 == sd.handed_out, "a learning sweep deferred after the free chain's pointer was handed out")
        if k in "LFIN" and other_owed:
            self._advanced_owed.add(self.active)
            if len(self._advanced_owed) == 2:
                self.cov["pair_advance_owed"] = True
        # ---- the static conditions of the coverage test
        if k == "I":
            self._since_i = False
            self._i_run += 1
            if self._i_run >= 3:
                self.cov["three_i"] = True
        elif k in "SAB":
            if self._since_i is not None:
                self._since_i = True
            self._i_run = 0
        elif k in "LF":
            if self._since_i:
                self.cov["i_then_weights_then_l"] = True
            self._since_i, self._i_run = None, 0
        elif k == "N":
            self._since_i, self._i_run = None, 0

    def _learned(self, sd, deferred_before, batches):
        sd.sweep += 1
        sd.cur *= DECAY
        sd.owed = sd.counters()[1] > deferred_before      # (a sweep that does not defer drops what was owed)

    def _pieces(self, sd, force, pack, host_write):
        """parity.learn_sweep_both with the sweep in pieces under a forced plan; host_write: new weights through the
        setter between the first update's accumulation and that update (a multi-GPU driver's order of calls is its
        own: tests/test_large_super_tiles.py) -- the draws accumulated so far saw the old weights, the update starts
        from the new ones"""
        s, o = sd.s, sd.o
        batches, n_chunks, _ = s.sgd_plan(sd.cur, force)
        self.check(batches == force, "sgd_plan(force_batches=%d) planned %d" % (force, batches))
        chunk_off = s.sgd_chunks(n_chunks)
        hess = None
        if batches > 1 and s.device_buffer(dwx.BUF_TSTATIC_PLAN)[1] == 0:
            hess = o.sched_curvature(self.order)
        if batches > 1 and sd.owed:
            self.cov["split_f_owed"] = True
        info = self.g.info
        if pack:
            self.check(info.grad_shift > 0, "G on a graph whose grad_shift does not allow it")
        for c in range(n_chunks):
            s.sgd_accumulate(c)
            sl = self.order[int(chunk_off[c, 0]):int(chunk_off[c, 1])]
            o.sched_accumulate(sl, np.array([0, len(sl)], np.uint64), sd.seed, sd.sweep)
            if batches > 1 or c + 1 == n_chunks:
                if host_write:
                    w = s.weights + self.rng.normal(0.0, 0.25, s.W)
                    s.weights = w
                    o.weights[:] = w
                    host_write = False
                if pack:
                    # (one rank: include/dwx.h's bounds at dwx_graph_info.grad_shift and dwx_grad_pack_async)
                    bits = 16 if info.max_records_per_weight * info.grad_unit_max < 2 ** 15 and sd.sweep % 2 == 0 else 32
                    self.check(info.max_records_per_weight * info.grad_unit_max < 2 ** 31, "counts beyond 32 bits")
                    s.grad_pack(info.grad_shift, bits)
                    s.grad_unpack(info.grad_shift, bits)
                s.sgd_apply()
                o.sched_apply(sd.cur, hess)
        s.sgd_finish()
        s.wait()            # (also the pack's check: every sum a multiple of 2^shift, every count inside the width)
        return batches

    def _oracle_average(self, sd, summed, n):
        # average_weights_kernel's contract (include/dwx.h at dwx_average_weights_async): weights /= n_replicas, fixed
        # weights restored verbatim
        fixed = np.asarray(self.raw.w_is_fixed) != 0
        sd.o.weights[:] = np.where(fixed, np.asarray(self.raw.w_initial_value, np.float64), summed / float(n))

    def _oracle_sweeps(self, sd, n):
        o, raw = sd.o, self.raw
        for _ in range(n):
            if sd.rb_on:
                from test_rao_blackwell import _conditional
                o.sched_sample(self.order[:0], np.array([0, 0], np.uint64), sd.seed, 0)     # (f32 sampling weights from here on)
                for L in range(len(self.off) - 1):
                    sl = self.order[int(self.off[L]):int(self.off[L + 1])]
                    for v in sd.rb_pick[L]:
                        c = _conditional(o, raw, v)
                        sd.rb_expected[self.base[v]:self.base[v] + len(c)] += c
                    o.sched_sample(sl, np.array([0, len(sl)], np.uint64), sd.seed, sd.sweep)
                sd.rb_n += 1
            else:
                o.sched_sample(self.order, self.off, sd.seed, sd.sweep)
            if sd.trace_on:
                sd.ring.append((sd.sweep, o.assignments("evid")[:self.n_owned].astype(np.uint8)))
                sd.ring = sd.ring[-sd.trace_cap:]
            sd.sweep += 1

    def _set_assignments(self, sd, chain):
        a = np.array(sd.o.assignments(chain))
        cand = np.arange(self.raw.num_variables) if chain == "f" else np.flatnonzero(self.role == 0)
        pick = self.rng.choice(cand, min(50, len(cand)), replace=False)
        a[pick] = self.rng.integers(0, self.card[pick])
        name = "free" if chain == "f" else "evid"
        sd.s.set_assignments(name, a)
        sd.o.assignments(name)[:] = a

    def _halo(self, sd, halo, mask):
        vids, h = halo["vids"], halo["h"]
        n = len(vids)
        top = int(self.card[vids].max())
        bits = 1 if top <= 2 else (8 if top <= 256 else 32)          # include/dwx.h at dwx_halo_message_bytes
        block = (n * bits + 63) // 64 * 8
        chains = [c for c, bit in (("free", 1), ("evid", 2)) if mask & bit]
        self.check(h.message_bytes(mask) == block * len(chains), "halo message bytes")
        ptr, nbytes = h.buffer()
        self.check(nbytes >= block * len(chains), "halo buffer size")
        h.pack(mask); sd.s.wait()
        got = np.zeros(block * len(chains), np.uint8)
        self.lib.check(self.lib.L.dwx_buffer_copy(sd.s.h, got.ctypes.data, ptr, len(got), 0))
        new = np.zeros_like(got)
        for i, chain in enumerate(chains):
            blk = got[i * block:(i + 1) * block]
            if bits == 1:
                vals = np.unpackbits(blk, bitorder="little")[:n]
            else:
                vals = blk.view(np.uint8 if bits == 8 else np.uint32)[:n]
            self.check(np.array_equal(vals.astype(np.uint64), sd.o.assignments(chain)[vids]), "halo pack, %s chain" % chain)
            # what a peer sends: any value on the free chain and on ghosts; the evidence chain of an owned evidence
            # variable keeps its value
            fresh = self.rng.integers(0, self.card[vids]).astype(np.uint64)
            if chain == "evid":
                keep = (self.role[vids] != 0) & (vids < self.n_owned)
                fresh[keep] = sd.o.assignments(chain)[vids][keep]
            out = new[i * block:(i + 1) * block]
            if bits == 1:
                packed = np.packbits(fresh.astype(np.uint8), bitorder="little")
                out[:len(packed)] = packed
            elif bits == 8:
                out[:n] = fresh.astype(np.uint8)
            else:
                out.view(np.uint32)[:n] = fresh.astype(np.uint32)
            halo["fresh_" + chain] = fresh
        self.lib.check(self.lib.L.dwx_buffer_copy(sd.s.h, ptr, new.ctypes.data, len(new), 1))
        h.unpack(mask); sd.s.wait()
        for chain in chains:
            sd.o.assignments(chain)[vids] = halo["fresh_" + chain]

    # -------------------------------------------------------------------- observers
    def _read(self, sd, which):
        s, o = sd.s, sd.o
        self.check(s.sweep == sd.sweep, "sweep counter %d, the model's %d" % (s.sweep, sd.sweep))
        for letter in which:
            f0 = sd.counters()[0]
            if letter == "f":
                self.check(np.array_equal(s.assignments("free"), o.assignments("free")), "free chain")
            elif letter == "e":
                self.check(np.array_equal(s.assignments("evid"), o.assignments("evid")), "evidence chain")
            elif letter == "t":
                t, n = s.tallies()
                self.check(np.array_equal(t, o.tallies[:len(t)]), "tallies")
                self.check(np.array_equal(n, o.nsamples), "nsamples")
            elif letter == "w":
                self.check(np.allclose(s.weights, o.weights, rtol=WTOL, atol=WTOL), "weights")
            elif letter == "r":
                self._read_trace(sd)
            elif letter == "b":
                self._read_rb(sd)
            elif letter in "sz" and self.case["expect"] is not None:
                chain = "free" if letter == "s" else "evid"
                want = self.case["expect"].scores(s.weights, np.array(o.assignments(chain), np.int64)[None])[0]
                got = s.score(chain)
                self.check(got == want, "score(%s) %r, the integer sum's %r" % (chain, got, want))
            if sd.counters()[0] > f0:
                sd.owed = False
                if letter in "fs":
                    self.cov["flush_by"].add("free_read")

    def _read_trace(self, sd):
        s = sd.s
        if not sd.trace_ever:
            return
        cnt, cap, ids = s.trace_info()
        self.check(cap == sd.trace_cap, "trace capacity %d, the model's %d" % (cap, sd.trace_cap))
        self.check(ids.tolist() == [i for i, _ in sd.ring], "trace ids %s, the history's %s" % (ids.tolist(), [i for i, _ in sd.ring]))
        if not cnt:
            return
        want = np.stack([x for _, x in sd.ring])
        got_ids, tr = s.trace()
        self.check(got_ids.tolist() == ids.tolist() and np.array_equal(tr, want), "trace planes")
        # the indicator series of every value row, from the MODEL's history
        from test_trace_diagnostics import _rows, _same, _transcription, MARGIN
        x, have = _rows(s, want)
        self.check(have.all(), "value rows without an owned variable")
        import test_trace_cooccurrence as cooc
        R = x.shape[1]
        a, b = self.rng.integers(0, R, 200), self.rng.integers(0, R, 200)
        a[:3], b[:3] = [0, R - 1, 0], [R - 1, R - 1, 0]
        cooc._check(s, x, a, b)
        if cnt > 2:
            cooc._check(s, x, a, b, 1, cnt - 1)
        if cnt < 4:             # include/dwx.h at dwx_trace_diagnostics: fewer than 4 entries held is DWX_E_INVALID
            return
        rhat, ess, flags, summ = s.trace_diagnostics(max_lag=64)
        self.check(summ["n_entries"] == cnt and summ["contiguous"] == int(np.all(np.diff(ids.astype(np.int64)) == 1)), "diagnostics summary")
        t_rhat, t_ess, t_flags, margin = _transcription(x, 64)
        self.check(np.array_equal(flags, t_flags), "diagnostics flags")
        _same(rhat, t_rhat, "rhat against the transcription")
        # (tests/test_trace_diagnostics.py leaves the rows on Geyer's cut out and bounds their share at 0.1 % of a
        # long trace; over the 4 or 5 entries held here a pair sum of exactly 0 is common, so the share is not bounded)
        clear = ~(margin < MARGIN)
        _same(ess[clear], t_ess[clear], "ess against the transcription")
        xf = x.astype(np.float64)[None]
        _same(rhat, diagnostics.split_rhat(xf), "rhat against diagnostics.split_rhat")
        some = np.flatnonzero(clear & ((flags & 2) == 0))[:300]         # (diagnostics.ess is a Python loop per row)
        if len(some):
            _same(ess[some], diagnostics.ess(xf[:, :, some]), "ess against diagnostics.ess")

    def _read_rb(self, sd):
        if not sd.rb_ever:
            return
        from test_rao_blackwell import BOUND, TWO32
        rb, ns = sd.s.rb_sums()
        self.check(np.array_equal(ns, sd.o.nsamples), "rb nsamples")
        err = np.abs(rb.astype(np.float64) / TWO32 - sd.rb_expected[:len(rb)])[sd.rb_checked[:len(rb)]]
        worst = float(err.max()) if len(err) else 0.0
        self.check(worst <= max(sd.rb_n, 1) * BOUND, "rb sums: largest error %.3g over %d sweeps" % (worst, sd.rb_n))
        rows_sampled = np.zeros(len(rb), bool)
        for v in np.flatnonzero(self.sampled).tolist():
            rows_sampled[self.base[v]:self.base[v] + self.rows[v]] = True
        self.check(not rb[~rows_sampled].any(), "rb rows of variables that are not sampled must stay 0")
        if sd.rb_n == 0:
            self.check(not rb.any(), "rb sums without a sweep that accumulates")


def _token(op):
    k = op[0]
    if k == "F":
        return "F%d%s%s" % (op[1], "G" if op[2] else "", "S" if op[3] else "")
    if k == "R":
        return "R:" + op[1]
    return k + "".join(str(x) for x in op[1:])
