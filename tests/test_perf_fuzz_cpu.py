"""Whole performances without a GPU: tests/perf_fuzz.py's scripts on tests/perf_model.py's composed model alone.

  * the model agrees with the oracle: after every block the envelope clocks oracle.cpuref left in the bank are the ones the model's
    stamps imply (Stage.block asserts it), and increments stay in the normal fp32 range (Stage.normal).  This is weaker than
    tests/test_pedal_cpu.py's scenes: the shadow clocks are fed by the same model calls that stamp the bank, so the check shows that
    the stamps reach the bank once and the oracle leaves them alone; of the flags only "a note struck in the performance and not
    released is active" is held -- the converse (a release that ran out leaves the note inactive) did not hold on every voice of
    these banks and is not asserted;
  * coverage, counted from the model's state and result words: every call kind in every seed, every listed interaction in every
    configuration and in at least two seeds, at most a quarter of a seed's calls inert;
  * the fuzz bites: each wrong model (a) .. (g) ends at least one default performance with another digest;
  * the same seed gives the same script and the same digest twice.
"""
from collections import Counter

import numpy as np
import pytest

import perf_fuzz as PF
import perf_model as PMD

NAMES = tuple(PF.CONFIGS)


def run(name, seed, wrong=""):
    cfg = PF.CONFIGS[name]
    bank, tables, g = PF.make_bank(cfg, seed)
    script = PF.performance(seed, cfg)
    st = PMD.Stage(bank, tables, g, cfg.K, cfg.vmask, cfg.mmask, wrong)
    PMD.perform(st, script)
    return st, script


@pytest.fixture(scope="module")
def right():
    """every default performance on the right model, once: {(configuration, seed): (stage, script)}"""
    return {(name, seed): run(name, seed) for name in NAMES for seed in PF.SEEDS}


def test_scripts_keep_to_specified_input(right):
    for (name, seed), (st, script) in right.items():
        PF.check_input(script)
        assert [b["frames"] for b in script if b["frames"] not in PF.FRAMES] == []
        assert {b["frames"] for b in script} == set(PF.FRAMES), (name, seed)


def test_every_call_kind_in_every_seed(right):
    for (name, seed), (st, script) in right.items():
        kinds = Counter(o.kind for o in st.log)
        print(f"{name} seed {seed}: {len(st.log)} calls, {dict(kinds)}")
        assert set(kinds) == set(PF.KINDS), (name, seed, sorted(set(PF.KINDS) - set(kinds)))


def test_every_interaction_is_reached(right):
    seeds = {what: set() for what in PMD.INTERACTIONS}
    for name in NAMES:
        total = Counter()
        for seed in PF.SEEDS:
            ev = right[(name, seed)][0].events
            for what in PMD.INTERACTIONS:
                if ev[what]:
                    total[what] += ev[what]
                    seeds[what].add((name, seed))
        print(f"{name}: " + ", ".join(f"{what} {total[what]}" for what in PMD.INTERACTIONS))
        missing = [what for what in PMD.INTERACTIONS if not total[what]]
        assert not missing, f"{name}: never reached over the seed set: {missing}"
    for what, where in seeds.items():
        print(f"{what}: {len(where)} performances")
        assert len({s for _, s in where}) >= 2, (what, sorted(where))


def test_at_most_a_quarter_of_the_calls_is_inert(right):
    for (name, seed), (st, script) in right.items():
        inert = [o.kind for o in st.log if o.inert]
        share = len(inert) / len(st.log)
        print(f"{name} seed {seed}: {len(inert)} of {len(st.log)} calls inert ({100 * share:.1f} %): {dict(Counter(inert))}")
        assert share <= 0.25, (name, seed, share)


def test_the_fuzz_bites(right):
    """each wrong model is told apart by at least one default seed"""
    caught = {}
    for w in PMD.WRONG:
        for name in NAMES:
            for seed in PF.SEEDS:
                if run(name, seed, w)[0].digest() != right[(name, seed)][0].digest():
                    caught.setdefault(w, []).append((name, seed))
            if w in caught:
                break                                                             # (one configuration that catches it is enough)
        print(f"({w}) {PMD.WRONG[w]}: caught by {caught.get(w)}")
    assert set(caught) == set(PMD.WRONG), f"caught by no seed: {sorted(set(PMD.WRONG) - set(caught))}"


def test_the_same_seed_twice(right):
    for name in NAMES:
        a, sa = run(name, 3)
        b, sb = right[(name, 3)]
        assert a.digest() == b.digest()
        assert [(k, sorted(kw)) for blk in sa for k, kw in blk["calls"]] == [(k, sorted(kw)) for blk in sb for k, kw in blk["calls"]]
        assert [o.res for o in a.log] == [o.res for o in b.log]
        assert all(np.array_equal(x.assigned, y.assigned) for x, y in zip(a.log, b.log) if x.assigned is not None)


# ---------------------------------------------------------------------------------------------- the composition itself

def test_the_glide_model_moves_the_truths_increments():
    """one array: a glide start and an advance change truth['voice_phase_inc'], which the oracle then renders"""
    import glide_model as GM
    cfg = PF.CONFIGS["plain"]
    bank, tables, g = PF.make_bank(cfg, 0)
    st = PMD.Stage(bank, tables, g, cfg.K, cfg.vmask, cfg.mmask)
    st.lists[-1] = np.array([40], np.int32)
    st.tag_slots(-1, [5])
    struck = st.truth["voice_phase_inc"][40]
    assert st.glide_tags([GM.Glide(GM.FROM_SCALE, 2.0, 0.5, 0.25)], 0, cfg.n, [5]).res == [1, 0, 0]
    assert st.truth["voice_phase_inc"][40] == struck * np.float32(0.25)
    assert st.glide_advance(0, cfg.n, 64).res == [1, 0] and st.truth["voice_phase_inc"][40] == struck * np.float32(0.5)
    assert st.glide_advance(0, cfg.n, 64).res == [0, 1] and st.truth["voice_phase_inc"][40] == struck


def test_the_planners_rule_pins_in_place_blocks(right):
    """plain2 is there for the motion-list bound: in every performance the in-place rule pins at least MIN_IN_PLACE blocks to the
    in-place path, and over the seeds such blocks lie behind stamp_match, pedal-ups, AMP sweeps and per-note velocities."""
    behind = Counter()
    for seed in PF.SEEDS:
        st = right[("plain2", seed)][0]
        want = PMD.in_place_verdicts(st)
        print(f"plain2 seed {seed}: {want}")
        assert sum(1 for w in want if w) >= PF.MIN_IN_PLACE and want[0] is False
        for b, w in enumerate(want):
            if w:
                behind.update(set(st.fronts[b]["kinds"]))
    print(dict(behind))
    assert all(behind[k] for k in ("stamp_match", "pedal_up", "ctl_match", "ctl_tags_each", "release_tags_pedal", "note_on_channel")), behind


def test_a_tag_clears_both_arrays():
    """The one tag rule on a slot that is pending AND gliding; each wrong model leaves its own array alone."""
    import glide_model as GM
    cfg = PF.CONFIGS["patch"]
    for wrong, pedal_left, glide_left in (("", False, False), ("a", True, False), ("b", False, True)):
        bank, tables, g = PF.make_bank(cfg, 0)
        st = PMD.Stage(bank, tables, g, cfg.K, cfg.vmask, cfg.mmask, wrong)
        st.lists[-1] = np.array([8, -1, 16], np.int32)
        st.tag_slots(-1, [5, 6, 7])
        st.pedal[8] = PMD.PENDING
        assert st.glide_tags([GM.Glide(GM.FROM_SCALE, 1.01, 0.99, 0.5)], 0, 64, [5]).res == [4, 0, 0]
        st.tag_slots(-1, [9, 6, 7])
        assert bool(st.pedal[8]) == pedal_left and bool(st.glide[8:12].any()) == glide_left, wrong
        assert st.events["theft of a pending slot"] == st.events["theft of a gliding slot"] == 1
