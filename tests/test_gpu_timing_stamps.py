"""-m gpu: the plan group (which = 0 of lsc_set_timing / lsc_kernel_times_ms) timed by clock stamps that its kernels write themselves.
One lane of every workgroup of the group's first launch folds the device's constant-rate clock into the slot's begin word (atomic
minimum), one lane of every workgroup of its last launch into its end word (atomic maximum); the launches are plain launches, and the
host reads the slots with one copy on query.  Stamps must change no result bit, every sample must be a positive time that fits inside
the host's wall clock around the ticks, the stamped span must agree with what the dispatch-bound events of the same launches read
(LSC_TIMING_EVENTS=1, the other arm), and a context whose slots are used up goes on with events, in launch order.  Every test also
asserts where its samples came from (kernel_samples_stamped): a quiet fall-back to events fails here, not only in the benchmark.

The shapes and the harness are those of test_gpu_timing_dispatch.py (which runs on the default arm, the stamps, as it stands)."""
import numpy as np
import pytest

from test_gpu_timing_dispatch import NAMES, Run, assert_samples, circle8, fly
from harness import assert_same_flights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import lsc_planner_amd as L
    return L


def _cfg(L, m, **kw):
    """the planner's configuration for the M = 5 library, or for the M = 4 one (dt 0.5, horizon 2.0: liblsc_hip_m4.so)"""
    if m == 4:
        L.load_library(4)
        kw.update(dt=0.5, horizon=2.0)
    return L.PlannerConfig(**kw)


@pytest.mark.parametrize("m", [5, 4])
def test_stamped_ticks_plan_the_same_bits_and_fit_the_wall_clock(L, m):
    """8-agent circle swap, 6 fused ticks: the one launch of a tick stamps both words of its slot."""
    timed, plain = Run(L, circle8(L), _cfg(L, m)), Run(L, circle8(L), _cfg(L, m))
    try:
        assert timed.pl.M == m
        timed.pl.set_timing(True)
        a, wall = fly([timed], 6)
        b, _ = fly([plain], 6)
        assert_same_flights(a, b, NAMES, "stamped vs untimed")
        assert_samples(timed.pl, 0, 6, wall)
        assert timed.pl.kernel_samples_stamped() == 6
        assert len(plain.pl.kernel_times_ms(0)) == 0 and plain.pl.kernel_samples_stamped() == 0
        timed.pl.set_timing(True)                    # again: the count restarts, and the slots are armed again
        assert len(timed.pl.kernel_times_ms(0)) == 0 and timed.pl.kernel_time_ms(0) == (0.0, 0)
        assert timed.pl.kernel_samples_stamped() == 0
        _, wall = fly([timed], 2)
        assert_samples(timed.pl, 0, 2, wall)
        assert timed.pl.kernel_samples_stamped() == 2
    finally:
        timed.pl.close()
        plain.pl.close()


def test_stamps_agree_with_the_events_of_the_same_launches(L, monkeypatch):
    """The same mission and ticks on a context timed by events (LSC_TIMING_EVENTS=1) and on one timed by stamps.  The stamped span lies
    inside the dispatch: its median may exceed the events' by at most 10 % (two separate runs of a ~25 us kernel), and is at least half of
    it (a wrong clock rate is a factor of 10 or 1000, a stop in front of its start is negative, a launch is not half of this kernel)."""
    monkeypatch.setenv("LSC_TIMING_EVENTS", "1")
    events = Run(L, circle8(L))
    monkeypatch.delenv("LSC_TIMING_EVENTS", raising=False)
    stamps = Run(L, circle8(L))
    try:
        events.pl.set_timing(True)
        stamps.pl.set_timing(True)
        a, wall_e = fly([events], 6)
        b, wall_s = fly([stamps], 6)
        assert_same_flights(a, b, NAMES, "events vs stamps")
        ke, ks = assert_samples(events.pl, 0, 6, wall_e), assert_samples(stamps.pl, 0, 6, wall_s)
        assert events.pl.kernel_samples_stamped() == 0 and stamps.pl.kernel_samples_stamped() == 6
        me, ms_ = float(np.median(ke)), float(np.median(ks))
        print(f"event samples (ms) {ke.tolist()}\nstamp samples (ms) {ks.tolist()}\nmedians: events {me:.6f} stamps {ms_:.6f} ratio {ms_ / me:.4f}")
        assert ms_ <= 1.10 * me, (ms_, me)
        assert ms_ >= 0.5 * me, (ms_, me)
    finally:
        events.pl.close()
        stamps.pl.close()


@pytest.mark.parametrize("m", [5, 4])
def test_begin_on_the_plan_kernel_end_on_the_hand_over_launch(L, monkeypatch, m):
    """reset_threshold 0.15 with the hand-over launch kept (LSC_GENERAL_HANDOVER): the plan kernel stamps the begin, lsc_general_kernel --
    whose workgroups leave at once -- the end."""
    cfg = lambda: _cfg(L, m, reset_threshold=0.15)
    monkeypatch.setenv("LSC_GENERAL_HANDOVER", "1")
    timed, plain = Run(L, circle8(L), cfg()), Run(L, circle8(L), cfg())
    monkeypatch.delenv("LSC_GENERAL_HANDOVER", raising=False)
    try:
        assert timed.pl.M == m
        timed.pl.set_timing(True)
        a, wall = fly([timed], 6)
        b, _ = fly([plain], 6)
        assert_same_flights(a, b, NAMES, "stamped vs untimed, hand-over launch")
        assert_samples(timed.pl, 0, 6, wall)
        assert timed.pl.kernel_samples_stamped() == 6
    finally:
        timed.pl.close()
        plain.pl.close()


def _swarm512(L):
    return L.random_swarm(512, world=(-14, -14, 0, 14, 14, 5), seed=20260930, min_sep=0.5)


def test_neighbour_build_query_and_throughput_kernel_ride_on_events(L, monkeypatch):
    """512 agents with the neighbour lists forced, 2 ticks: build -> query -> plan.  A shard of more agents than CUs takes the throughput
    kernels, which stamp nothing (their text is the untimed kernels'): the group is timed by events, start on the build, stop on the plan."""
    monkeypatch.setenv("LSC_NEIGH_ALWAYS", "1")
    timed, plain = Run(L, _swarm512(L), L.PlannerConfig()), Run(L, _swarm512(L), L.PlannerConfig())
    monkeypatch.delenv("LSC_NEIGH_ALWAYS", raising=False)
    try:
        timed.pl.set_timing(True)
        a, wall = fly([timed], 2)
        b, _ = fly([plain], 2)
        assert_same_flights(a, b, NAMES, "timed vs untimed, neighbour lists")
        assert_samples(timed.pl, 0, 2, wall)
        assert timed.pl.kernel_samples_stamped() == 0
        lists = timed.pl.neighbour_counts()
        assert lists is not None and (lists >= 0).any(), "the lists are meant to be in use"
    finally:
        timed.pl.close()
        plain.pl.close()


def test_begin_on_the_neighbour_build_end_on_the_plan_kernel(L, monkeypatch):
    """The first 256 of the same 512 agents as a shard (one agent per CU: the latency build), lists forced, the first tick: the neighbour
    build stamps the begin, the query neither, the group's last launch (the plan kernel, or the second pass behind it) the end."""
    monkeypatch.setenv("LSC_NEIGH_ALWAYS", "1")
    timed, plain = Run(L, _swarm512(L), L.PlannerConfig()), Run(L, _swarm512(L), L.PlannerConfig())
    monkeypatch.delenv("LSC_NEIGH_ALWAYS", raising=False)
    try:
        for r in (timed, plain):
            r.pl.set_shard(0, 256)
        timed.pl.set_timing(True)
        a, wall = fly([timed], 1)
        b, _ = fly([plain], 1)
        assert_same_flights(a, b, NAMES, "stamped vs untimed, neighbour lists, a shard of 256")
        assert_samples(timed.pl, 0, 1, wall)
        assert timed.pl.kernel_samples_stamped() == 1
        lists = timed.pl.neighbour_counts()
        assert lists is not None and (lists >= 0).any(), "the lists are meant to be in use"
    finally:
        timed.pl.close()
        plain.pl.close()


def test_batch_launch_stamps_one_slot_of_the_first_context(L):
    """Two 8-agent swarms in one launch per tick, 4 ticks: both swarms' workgroups stamp the slot of context 0; the plans are those of
    each swarm ticking alone."""
    mk = lambda: [Run(L, circle8(L, 3.0)), Run(L, circle8(L, 2.6))]
    bat, solo = mk(), mk()
    try:
        bat[0].pl.set_timing(True)
        a, wall = fly(bat, 4, batch_L=L)
        b, _ = fly(solo, 4)
        assert_same_flights(a, b, NAMES, "batched and stamped vs alone and untimed")
        assert_samples(bat[0].pl, 0, 4, wall)
        assert bat[0].pl.kernel_samples_stamped() == 4
        assert len(bat[1].pl.kernel_times_ms(0)) == 0 and bat[1].pl.kernel_samples_stamped() == 0
    finally:
        for r in bat + solo:
            r.pl.close()


def test_samples_beyond_the_slots_come_from_events(L, monkeypatch):
    """LSC_TIMING_SLOTS=4, 6 ticks: four stamped samples, then two from events, one list in launch order; re-arming gives the slots back."""
    monkeypatch.setenv("LSC_TIMING_SLOTS", "4")
    timed = Run(L, circle8(L))
    monkeypatch.delenv("LSC_TIMING_SLOTS", raising=False)
    plain = Run(L, circle8(L))
    try:
        timed.pl.set_timing(True)
        a, wall = fly([timed], 6)
        b, _ = fly([plain], 6)
        assert_same_flights(a, b, NAMES, "four slots vs untimed")
        assert_samples(timed.pl, 0, 6, wall)
        assert timed.pl.kernel_samples_stamped() == 4          # (the last two came from events)
        timed.pl.set_timing(True)
        assert len(timed.pl.kernel_times_ms(0)) == 0
        _, wall = fly([timed], 5)
        assert_samples(timed.pl, 0, 5, wall)
        assert timed.pl.kernel_samples_stamped() == 4
    finally:
        timed.pl.close()
        plain.pl.close()
