"""Request isolation at the engine level: the result of a job is a function of that job alone.  Every assertion is torch.equal between
an engine that has run other jobs and one that has not (tests/isolation_cases.py: the probes P1 - P4, the histories, the explicit and
the minimal preamble; INTEGRATION.md "State that outlives a run": the inventory the preambles are taken from).  The engines are built
once per module and every fresh result once per probe, after two fresh engines have agreed on it."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import isolation_cases as I  # noqa: E402
from isolation_cases import DEV, HISTORIES, P1, P2, P3, P4, PROBES  # noqa: E402


class Bench:
    """The reused engines, their cases, the other job's cases, the fresh results and what the histories since the last probe left."""

    def __init__(self):
        self.case = {w: I.make_case(w) for w in ("xl", "sd")}
        self.other = {w: I.make_case(w, seed=101) for w in ("xl", "sd")}
        self.eng = {w: I.build_engine(self.case[w]) for w in ("xl", "sd")}
        self.dirty = {"xl": set(), "sd": set()}
        self.fresh, self.agree = {}, {}
        for p in PROBES.values():
            got = []
            for _ in range(2):                                # two engines nothing else has used: they must agree before either is trusted
                e = I.build_engine(self.case[p.which])
                try:
                    got.append(I.run_probe(e, self.case[p.which], p, "fresh"))
                finally:
                    e.close()
            self.fresh[p.name], self.agree[p.name] = got[0], I.first_difference(got[1], got[0])

    def close(self):
        for e in self.eng.values():
            e.close()

    def history(self, which, name):
        self.dirty[which] |= set(HISTORIES[name](self.eng[which], self.case[which], self.other[which]))

    def probe(self, p, mode, after):
        """Runs probe p on the reused engine and fails, naming the histories and the first differing stream, unless it equals the fresh result."""
        dirty = tuple(sorted(self.dirty[p.which]))
        got = I.run_probe(self.eng[p.which], self.case[p.which], p, mode, dirty)
        self.dirty[p.which] = set()
        bad = I.first_difference(got, self.fresh[p.name])
        if bad is not None:
            d = (got[bad].double() - self.fresh[p.name][bad].double()).abs().max().item()
            pytest.fail(f"{p.name} with the {mode} preamble after [{after}] differs from a fresh engine: first differing stream: {bad} "
                        f"(max |difference| {d:.3e})", pytrace=False)


@pytest.fixture(scope="module")
def bench():
    b = Bench()
    yield b
    b.close()


@pytest.mark.parametrize("probe", list(PROBES))
def test_two_fresh_engines_agree(bench, probe):
    """Determinism first: a difference below is a leak only if two engines that nothing else has used give the same bits."""
    assert bench.agree[probe] is None, f"{probe}: two fresh engines differ in {bench.agree[probe]}"
    assert all(bool(torch.isfinite(t.float()).all()) for t in bench.fresh[probe].values())


PAIRS = [(p.name, h) for p in PROBES.values() for h in I.histories_of(p.which)]


@pytest.mark.parametrize("probe,history", PAIRS, ids=[f"{p}-after-{h}" for p, h in PAIRS])
def test_probe_after_a_history_equals_the_fresh_engine(bench, probe, history):
    """The history, then the probe with every option set by name; the history again, then the probe with nothing but the inventory's
    clearing calls for what that history left.  Both equal the fresh engine's result, bit for bit."""
    p = PROBES[probe]
    for mode in ("explicit", "minimal"):
        bench.history(p.which, history)
        bench.probe(p, mode, history)


ORDERS = {"listed": lambda names: list(names), "reversed-interleaved": lambda names: list(names)[::-2] + list(names)[-2::-2]}


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("which", ["xl", "sd"])
def test_histories_accumulate_in_two_orders(bench, which, order):
    """Every history of the engine, one after the other, in two orders; after each one every probe of the engine with the minimal
    preamble, the probe that meets the history first rotating.  Nothing else cleans up: what a probe's inputs and the clearing calls
    do not reach stays for the next history and the next probe to meet."""
    names = ORDERS[order](I.histories_of(which))
    assert sorted(names) == sorted(I.histories_of(which))
    probes = [p for p in PROBES.values() if p.which == which]
    done = []
    for k, h in enumerate(names):
        bench.history(which, h)
        done.append(h)
        for p in probes[k % len(probes):] + probes[:k % len(probes)]:
            bench.probe(p, "minimal", " -> ".join(done))


@pytest.mark.parametrize("probe,option", [(p.name, o) for p, o, _ in I.TEETH])
def test_an_option_left_on_changes_the_probe(bench, probe, option):
    """Teeth: with the option a history turns on still on, the probe's result is NOT the fresh one - so the equalities of this module
    cannot hold merely because the option does nothing at this size.  Afterwards the explicit preamble restores the fresh bits."""
    p = PROBES[probe]
    apply = next(f for q, o, f in I.TEETH if q is p and o == option)
    eng, c = bench.eng[p.which], bench.case[p.which]
    I.prepare(eng, c, p, "explicit")
    apply(eng, c)
    got = p.run(eng, c)
    assert I.first_difference(got, bench.fresh[p.name]) is not None, f"{p.name}: {option} left on changes no bit of the result"
    bench.probe(p, "explicit", f"{option} left on")


@pytest.mark.parametrize("probe", [P1.name, P3.name])
def test_refused_calls_between_two_steps_change_nothing(bench, probe):
    """Refused calls in mid-sequence: one of every validating setter between step 1 and step 2 of the probe itself."""
    p = PROBES[probe]
    eng, c = bench.eng[p.which], bench.case[p.which]
    I.prepare(eng, c, p, "explicit")
    I.rich_steps(eng, c, [0])
    I.refused_calls(eng, c)
    I.rich_steps(eng, c, range(1, 3 if p is P1 else 5))
    bad = I.first_difference(I.read(eng, c), bench.fresh[p.name])
    assert bad is None, f"{p.name}: refused calls between two steps changed {bad}"


@pytest.mark.parametrize("sched,first,resume", [("pndm", 3, 0), ("dpm2", 2, 1), ("sde2", 2, 1)])
def test_set_schedule_alone_resets_the_solver(bench, sched, first, resume):
    """The inventory says set_schedule returns the multistep state to its default by itself.  A two-stage job on one engine - `first` plain
    steps, then set_schedule and nothing else, then the steps from index `resume` on - equals an engine that is handed the first stage's
    latents with set_latents (which resets too) behind the same set_schedule.  A resumed DPM run starts at index 1, where a stale history
    count would select the second-order update and read the first stage's x0."""
    eng, c = bench.eng["xl"], bench.case["xl"]
    s = I.schedule(sched, 4)
    n = len(s[1])

    def stage_one():
        I.prepare(eng, c, P2, "explicit")
        eng.set_schedule(*s)
        for i in range(first):
            eng.plain_step(i, c["gs"])

    def stage_two():
        for i in range(resume, n):
            eng.plain_step(i, c["gs"])
        return eng.read_latents(c["h"], c["w"])
    stage_one()
    mid = eng.read_latents(c["h"], c["w"]).clone()
    eng.set_schedule(*s)
    got = stage_two()
    stage_one()                                                # the same history in front of the reference run, then both resets
    eng.set_schedule(*s)
    eng.set_latents(mid)
    want = stage_two()
    assert torch.equal(got, want), f"{sched}: set_schedule alone left solver state behind (max |difference| {(got - want).abs().max().item():.3e})"
    assert not torch.equal(got, mid)


def test_smaller_grids_on_a_larger_engine(bench):
    """An engine built for 64 x 96 latents runs P1 at 32 x 32: its bits are those of the 32 x 32 engine (a capacity is not an input), and
    they stay after a step of a 32 x 48 grid and one of the full 64 x 96 grid on the same engine, with either preamble."""
    c = bench.case["xl"]
    others = [I.make_case("xl", 32, 48, seed=103), I.make_case("xl", 64, 96, seed=105)]
    got = []
    for _ in range(2):
        e = I.build_engine(c, 64, 96)
        got.append(I.run_probe(e, c, P1, "fresh"))
        if len(got) == 1:
            e.close()
    assert I.first_difference(got[1], got[0]) is None, "two fresh 64 x 96 engines differ"
    try:
        bad = I.first_difference(got[0], bench.fresh[P1.name])
        assert bad is None, f"P1 on a fresh 64 x 96 engine differs from the 32 x 32 engine in {bad}"
        for mode in ("explicit", "minimal"):
            for o in others:
                I.rich_inputs(e, o)
                I.start(e, o, I.schedule("euler", 3))
                I.rich_steps(e, o, [0])
            bad = I.first_difference(I.run_probe(e, c, P1, mode), bench.fresh[P1.name])
            assert bad is None, f"P1 ({mode}) after a 32 x 48 and a 64 x 96 step on the 64 x 96 engine differs in {bad}"
    finally:
        e.close()
