"""GPU: the output side of dg_encode_plan_run, as include/delta_gpu.h states it.

Every run writes into pad + output_bound + pad guard bytes, whatever out_cap it
is given, with spare guarded entries behind d_offsets and d_status; the input
arenas end at the last pair's last byte.  Every delta is compared exactly with
the oracle's (onepass, correcting) or the greedy model's.

a. containment: out_cap = output_bound and out_cap = the total exactly, d_out
   at every alignment; no byte outside [0, total) is written;
b. an out_cap one byte short of pair k: pairs k.. get DG_ERR_CAPACITY and write
   nothing, the offsets still count them, and nothing sticks to the plan;
c. one plan re-run on other bytes of its layout (tests/encode_plan_cases.py
   datasets), the automatic mode's stale routing hint included;
d. stream order without a host synchronisation: the run is enqueued before the
   copies that write its inputs have run;
e. the argument checks, and a context closed before its plans (the Python
   classes: the collector finalises them in any order).

The inputs' shapes (record counts on the tile boundaries, payload classes,
dense member chunks, tiles over the stages) are proven by
tests/test_encode_plan_cases_cpu.py.
"""
from __future__ import annotations

import pytest

import encode_plan_cases as C
import greedy_cases as G

pytestmark = pytest.mark.gpu

ONEPASS, CORRECTING = 1, 2
OK, INVALID_ARG, CAPACITY = 0, 1, 7
GUARD = 0xA5
PAD = 4096
SPARE = 8                          # guarded entries behind d_offsets and d_status
OFF_GUARD = -0x5A5A5A5A5A5A5A5B    # 0xA5A5... as int64
ST_GUARD = -0x5A5A5A5B

OTHER = [("correcting", 1), ("correcting", 1048573), ("greedy", 1)]   # LDS index build, global build, greedy


def _other_id(v):
    return f"{v[0]}_q{v[1]}" if v[0] != "greedy" else "greedy"


_EXPECT, _DATA = {}, {}


def expected(orc, algo, q, key, pairs):
    """The deltas of `pairs`, computed once per (algorithm, q, input set)."""
    k = (algo, q if algo != "greedy" else 0, key)
    if k not in _EXPECT:
        if algo == "greedy":
            _EXPECT[k] = [G.model_delta(orc, R, V, C.P) for R, V in pairs]
        else:
            a = ONEPASS if algo == "onepass" else CORRECTING
            _EXPECT[k] = [orc.encode(a, R, V, p=C.P, q=q) for R, V in pairs]
    return _EXPECT[k]


def small_pairs():
    return [(R, V) for _, R, V in C.small_layout_cases()]


def small_names():
    return [name for name, _, _ in C.small_layout_cases()]


def data(which):
    """The datasets of the small re-run layout and of the 8 x 160 KiB one."""
    if which not in _DATA:
        _DATA[which] = C.datasets(C.rerun_lengths() if which == "small" else C.auto_lengths(),
                                  seed=1 if which == "small" else 2)
    return _DATA[which]


class Run:
    """One encode plan over one layout.  load() writes the arenas (exactly the
    layout's bytes: they end with the last pair); run() gives the plan a fresh
    guarded output and guarded side arrays and reads everything back."""

    def __init__(self, torch, dg, ctx, algo, lay, q=1):
        self.torch, self.dg, self.ctx, self.lay = torch, dg, ctx, lay
        self.n = len(lay.lay)
        self.plan = dg.EncodePlan(ctx, algo, lay.lay, p=C.P, q=q)
        self.bound = self.plan.output_bound
        self.off = torch.empty(self.n + 1 + SPARE, dtype=torch.int64, device="cuda")
        self.st = torch.empty(self.n + SPARE, dtype=torch.int32, device="cuda")
        self.arena = None

    def device_arenas(self, pairs):
        torch = self.torch
        host = C.arenas(self.lay, pairs, fill=GUARD)
        assert len(host[0]) == self.lay.r_size > 0 and len(host[1]) == self.lay.v_size > 0
        return [torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda() for b in host]

    def load(self, pairs):
        new = self.device_arenas(pairs)
        if self.arena is None:
            self.arena = new
        else:   # the same device buffers, other bytes
            for a, b in zip(self.arena, new):
                a.copy_(b)
        self.torch.cuda.synchronize()
        return self

    def run(self, out_cap=None, shift=0, stream=0, before=None, d_ref=None, d_ver=None, d_out=None):
        torch = self.torch
        self.base = torch.full((PAD + self.bound + PAD,), GUARD, dtype=torch.uint8, device="cuda")
        self.off.fill_(OFF_GUARD)
        self.st.fill_(ST_GUARD)
        torch.cuda.synchronize()
        self.shift = shift
        self.out_cap = self.bound if out_cap is None else out_cap
        if before:
            before()
        self.plan.run(self.arena[0].data_ptr() if d_ref is None else d_ref,
                      self.arena[1].data_ptr() if d_ver is None else d_ver,
                      self.base.data_ptr() + PAD + shift if d_out is None else d_out,
                      self.out_cap, self.off.data_ptr(), self.st.data_ptr(), stream or self.ctx.stream)
        return self.read()

    def read(self):
        n = self.n
        self.torch.cuda.synchronize()
        raw = bytes(self.base.cpu().numpy())
        at = PAD + self.shift
        self.front, self.body = raw[:at], raw[at:]   # body: from d_out to the allocation's end
        offs, st = self.off.cpu().tolist(), self.st.cpu().tolist()
        assert offs[n + 1:] == [OFF_GUARD] * SPARE, "an offset past d_offsets[n]"
        assert st[n:] == [ST_GUARD] * SPARE, "a status past d_status[n - 1]"
        assert self.front == bytes([GUARD]) * at, "a byte before d_out"
        self.offs, self.status = offs[:n + 1], st[:n]
        return self

    def delta(self, i):
        return self.body[self.offs[i]:self.offs[i + 1]]

    def guard_from(self, at):
        """Every byte from d_out + at to the allocation's end is untouched."""
        rest = self.body[at:]
        if rest != bytes([GUARD]) * len(rest):
            bad = [i for i, b in enumerate(rest) if b != GUARD]
            raise AssertionError(f"{len(bad)} bytes written at d_out + {at + bad[0]} .. {at + bad[-1]} "
                                 f"(end of the written deltas: {at}, out_cap {self.out_cap})")

    def check(self, exp, names=None):
        """Statuses 0, the offsets packed and monotone, every delta exact,
        nothing written from the total on."""
        assert self.status == [OK] * self.n
        at = 0
        for i, e in enumerate(exp):
            assert self.offs[i] == at, (i, names[i] if names else None)
            assert self.delta(i) == e, (i, names[i] if names else None)
            at += len(e)
        assert self.offs[self.n] == at <= self.bound
        self.guard_from(at)
        return self


def _mode(request):
    return request.node.callspec.params["ctx_mode"]


def _check_members(request, plan, align):
    """An unaligned layout drops the LDS-window chain and the members with it;
    the small layouts' mean pair is far below automatic mode's 128 KiB."""
    assert plan.members == (_mode(request) == "members" and align == 16)


# ── a. containment ──────────────────────────────────────────────────────────

def _containment(run, exp, names):
    first = run.run().check(exp, names)
    offs, total = list(first.offs), first.offs[run.n]
    assert total <= run.bound
    for shift in (0, 1, 7, 13):   # the ABI asks no alignment of d_out
        for cap in (run.bound, total):
            if (shift, cap) == (0, run.bound):
                continue
            r = run.run(out_cap=cap, shift=shift).check(exp, names)
            assert r.offs == offs


@pytest.mark.parametrize("align", [16, 1])
@pytest.mark.parametrize("q", [1, 1048573])
def test_containment_onepass(dg, ctx_mode, orc, torch_cuda, request, q, align):
    pairs = small_pairs()
    run = Run(torch_cuda, dg, ctx_mode, "onepass", C.layout(pairs, align), q=q).load(pairs)
    _check_members(request, run.plan, align)
    _containment(run, expected(orc, "onepass", q, "small", pairs), small_names())


@pytest.mark.parametrize("variant", OTHER, ids=_other_id)
def test_containment(dg, ctx, orc, torch_cuda, variant):
    algo, q = variant
    pairs = small_pairs()
    run = Run(torch_cuda, dg, ctx, algo, C.layout(pairs, 16), q=q).load(pairs)
    _containment(run, expected(orc, algo, q, "small", pairs), small_names())


# ── b. an out_cap that fits only the first k pairs ──────────────────────────

def _tight(run, exp, names):
    n = run.n
    offs = list(run.run().check(exp, names).offs)
    chunks3 = names.index("dense_17")   # in member mode: a failing pair of several chunk jobs
    assert min(len(x) for x in small_pairs()[chunks3]) // C.CHUNK + 1 >= 3
    for k in sorted({0, 1, n // 2, n - 1, chunks3}):
        r = run.run(out_cap=offs[k + 1] - 1)
        assert r.status == [OK] * k + [CAPACITY] * (n - k), k
        assert r.offs == offs, k               # a failed pair's size is still counted
        for i in range(k):
            assert r.delta(i) == exp[i], (k, i, names[i])
        r.guard_from(offs[k])                  # a failed pair writes nothing, not even its header
    run.run().check(exp, names)                # no status or size sticks to the plan


@pytest.mark.parametrize("align", [16, 1])
@pytest.mark.parametrize("q", [1, 1048573])
def test_tight_out_cap_onepass(dg, ctx_mode, orc, torch_cuda, request, q, align):
    pairs = small_pairs()
    run = Run(torch_cuda, dg, ctx_mode, "onepass", C.layout(pairs, align), q=q).load(pairs)
    _check_members(request, run.plan, align)
    _tight(run, expected(orc, "onepass", q, "small", pairs), small_names())


@pytest.mark.parametrize("variant", OTHER, ids=_other_id)
def test_tight_out_cap(dg, ctx, orc, torch_cuda, variant):
    algo, q = variant
    pairs = small_pairs()
    run = Run(torch_cuda, dg, ctx, algo, C.layout(pairs, 16), q=q).load(pairs)
    _tight(run, expected(orc, algo, q, "small", pairs), small_names())


# ── c. one plan, other bytes of the same layout ─────────────────────────────

ORDER = ["edits", "unrelated", "edits", "shift", "same", "edits"]


def _rerun(run, orc, algo, q):
    ds = data("small")
    exp = {name: expected(orc, algo, q, "rerun_" + name, ds[name]) for name in set(ORDER)}
    assert len({tuple(e) for e in exp.values()}) == len(exp)
    for step, name in enumerate(ORDER):
        run.load(ds[name])
        r = run.run()
        assert r.status == [OK] * run.n, (step, name)
        for i, e in enumerate(exp[name]):
            assert r.delta(i) == e, (step, name, i)
        r.check(exp[name])


@pytest.mark.parametrize("q", [1, 257, 1048573])
def test_rerun_other_bytes_onepass(dg, ctx_mode, orc, torch_cuda, request, q):
    run = Run(torch_cuda, dg, ctx_mode, "onepass", C.layout(C.rerun_lengths(), 16), q=q)
    _check_members(request, run.plan, 16)
    _rerun(run, orc, "onepass", q)


@pytest.mark.parametrize("q", [1, 65537, 1048573])
def test_rerun_other_bytes_correcting(dg, ctx, orc, torch_cuda, q):
    """q = 1: every index built in LDS; 1048573: in global memory, nearly empty;
    65537: in global memory and, for the 64 KiB pair, half full, so that entries
    left by another run's bytes displace this run's (the global build only
    fills: launch_correcting_clear empties the indexes before it)."""
    _rerun(Run(torch_cuda, dg, ctx, "correcting", C.layout(C.rerun_lengths(), 16), q=q), orc, "correcting", q)


def test_rerun_on_a_stale_routing_hint(dg, orc, torch_cuda):
    """Automatic member mode reads its routing hint from the previous run: after
    a run that routed every pair to the plain chain, the next 15 run as plain
    plans whatever their bytes, and the 16th probes in member mode again."""
    ctx = dg.Context(0)
    ctx.set_limit(dg.LIMIT_ONEPASS_MEMBERS, dg.MEMBERS_AUTO)
    ds = data("auto")
    exp = {name: expected(orc, "onepass", 1, "auto_" + name, ds[name]) for name in ("edits", "shift")}
    assert exp["edits"] != exp["shift"]
    run = Run(torch_cuda, dg, ctx, "onepass", C.layout(C.auto_lengths(), 16), q=1)
    assert run.plan.members
    dev = {name: run.device_arenas(ds[name]) for name in exp}
    for step in range(18):   # shift first, then edits and shift in turn
        name = "edits" if step % 2 else "shift"
        run.arena = dev[name]
        torch_cuda.cuda.synchronize()
        run.run().check(exp[name])
        if step == 0:
            assert run.plan.run_modes == (1, 0)
    modes = run.plan.run_modes
    assert sum(modes) == 18 and modes[0] >= 2 and modes[1] >= 2, modes
    assert modes == (2, 16), modes   # runs 1 and 17 in member mode


# ── d. stream order without a host synchronisation ──────────────────────────

def _stream_order(torch, dg, ctx, orc, algo, members=None):
    ds = data("small")
    A, B = ds["edits"], ds["shift"]
    exp_a, exp_b = (expected(orc, algo, 1, "rerun_" + k, ds[k]) for k in ("edits", "shift"))
    assert all(a[9:25] != b[9:25] for a, b in zip(exp_a, exp_b))   # both CRCs differ
    run = Run(torch, dg, ctx, algo, C.layout(C.rerun_lengths(), 16), q=1).load(A)
    if members is not None:
        assert run.plan.members == members
    s = torch.cuda.Stream()
    run.run(stream=s.cuda_stream).check(exp_a)
    nxt = run.device_arenas(B)
    big = torch.zeros((2, 128 << 20), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def before():   # all on s, none waited for: the run is enqueued before its inputs are written
        with torch.cuda.stream(s):
            for _ in range(4):
                big[1].copy_(big[0])
            run.arena[0].copy_(nxt[0])
            run.arena[1].copy_(nxt[1])

    run.run(stream=s.cuda_stream, before=before).check(exp_b)


@pytest.mark.parametrize("mode", ["members", "chain"])
def test_stream_order_onepass(dg, orc, torch_cuda, mode):
    ctx = dg.Context(0)
    ctx.set_limit(dg.LIMIT_ONEPASS_MEMBERS, dg.MEMBERS_ON if mode == "members" else dg.MEMBERS_OFF)
    _stream_order(torch_cuda, dg, ctx, orc, "onepass", members=mode == "members")


def test_stream_order_correcting(dg, ctx, orc, torch_cuda):
    _stream_order(torch_cuda, dg, ctx, orc, "correcting")


# ── e. arguments ────────────────────────────────────────────────────────────

@pytest.mark.parametrize("algo", ["onepass", "correcting", "greedy"])
def test_arguments(dg, ctx, orc, torch_cuda, algo):
    empty = dg.EncodePlan(ctx, algo, [], p=C.P)
    assert empty.output_bound == 0 and empty.n == 0
    empty.run(0, 0, 0, 0, 0, 0)                      # DG_OK, null pointers and all
    empty.run(0, 0, 0, 0, 0, 0, ctx.stream)
    ds = data("small")
    run = Run(torch_cuda, dg, ctx, algo, C.layout(C.rerun_lengths(), 16), q=1).load(ds["edits"])
    r_ptr, v_ptr = run.arena[0].data_ptr(), run.arena[1].data_ptr()
    assert r_ptr % 16 == 0 and v_ptr % 16 == 0

    def code_of(call):
        try:
            call()
        except dg.DeltaError as e:
            return e.code
        return OK

    for kw in (dict(d_ref=r_ptr + 1), dict(d_ver=v_ptr + 8), dict(d_ref=r_ptr + 15, d_ver=v_ptr + 4)):
        assert code_of(lambda: run.run(**kw)) == INVALID_ARG
        run.read().guard_from(0)
        assert run.offs == [OFF_GUARD] * (run.n + 1) and run.status == [ST_GUARD] * run.n
    assert code_of(lambda: run.plan.run(r_ptr, v_ptr, 0, run.bound, run.off.data_ptr(), run.st.data_ptr(),
                                        ctx.stream)) == INVALID_ARG
    run.run().check(expected(orc, algo, 1, "rerun_edits", ds["edits"]))   # and the plan still runs


def test_context_closed_before_its_plans(dg, orc, torch_cuda):
    """A plan's destroy uses its context (its stream, its device), and Python
    finalises a context and its plans in any order once they are garbage
    together.  The context therefore takes its live plans along when it closes,
    and closing them afterwards does nothing."""
    ctx = dg.Context(0)
    lay = C.layout(C.rerun_lengths(), 16)
    run = Run(torch_cuda, dg, ctx, "onepass", lay, q=1).load(data("small")["edits"])
    run.run().check(expected(orc, "onepass", 1, "rerun_edits", data("small")["edits"]))
    plans = [run.plan, dg.EncodePlan(ctx, "correcting", lay.lay, p=C.P, q=1), dg.EncodePlan(ctx, "greedy", [], p=C.P)]
    assert len(ctx._plans) == len(plans)
    plans[1].close()                 # the usual order for one of them
    assert len(ctx._plans) == len(plans) - 1
    ctx.close()
    assert ctx.handle is None and not ctx._plans
    for p in plans:
        p.close()
        assert p.handle is None
    ctx.close()
