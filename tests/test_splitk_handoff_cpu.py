"""The checks of test_splitk_handoff_gpu.py, each shown to fail on the fault it exists for (the convention of test_parity_cpu.py), on
a toy emulation of the in-kernel split-K reduction (tests/handoff.py: FixupEmulation).  No GPU.

What this file records: a finisher that reads the PREVIOUS launch's fragment passes every test that re-launches the same inputs (the
design of the bit-identity tests of test_pp_gpu.py) and fails the alternating schedule at its first change of operand set."""
import pytest
import torch

import handoff as H


def _sets(em, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(em.M, em.K, generator=g), torch.randn(em.N, em.K, generator=g)) for _ in range(2)]


def _run(em, sets, schedule, fill):
    em.fill(fill)
    refs = [(em.reference(a, w),) for a, w in sets]
    outs = [(em.launch(*sets[s]),) for s in schedule]
    return outs, refs


@pytest.mark.parametrize("fill", ["zero", "nan"])
def test_clean_emulation_passes_both_schedules(fill):
    em = H.FixupEmulation()
    sets = _sets(em)
    for schedule in ((0,) * 6, H.SCHEDULE):
        outs, refs = _run(em, sets, schedule, fill)
        assert H.first_mismatch(outs, refs, schedule) is None
        H.assert_sequence(outs, refs, "clean", schedule)
        assert not bool(em.cnt.any())


def test_a_stale_fragment_passes_identical_relaunches_and_fails_the_alternating_schedule():
    """The fault needs a previous fragment to read, so the sequence starts from a workspace that a launch of the same operand set
    has already used -- what every bit-identity test of test_pp_gpu.py does when it repeats its launch."""
    for tile, s in ((0, 0), (3, 1)):
        em = H.FixupEmulation(fault=("stale", tile, s))
        sets = _sets(em)
        em.fault = None
        em.launch(*sets[0])  # the earlier launch whose fragment the fault then reads
        em.fault = ("stale", tile, s)
        same = (0,) * 6
        refs = [(em.reference(a, w),) for a, w in sets]
        outs = [(em.launch(*sets[i]),) for i in same]
        assert H.first_mismatch(outs, refs, same) is None, "identical re-launches cannot see a stale fragment: the old design's blind spot"
        outs = [(em.launch(*sets[i]),) for i in H.SCHEDULE]
        assert H.first_mismatch(outs, refs, H.SCHEDULE) == 1, "caught at the first X0 -> X1 transition"
        with pytest.raises(AssertionError, match="launch 1 of 6"):
            H.assert_sequence(outs, refs, "stale")


def test_a_stale_fragment_on_a_nan_filled_workspace_fails_the_first_launch():
    em = H.FixupEmulation(fault=("stale", 2, 0))
    outs, refs = _run(em, _sets(em), H.SCHEDULE, "nan")
    assert H.first_mismatch(outs, refs) == 0
    assert bool(torch.isnan(outs[0][0]).any())


@pytest.mark.parametrize("tile,s", [(0, 0), (1, 1), (3, 0)])
def test_a_fragment_read_before_it_is_written_fails_the_first_launch_under_the_nan_fill(tile, s):
    em = H.FixupEmulation(fault=("not_written", tile, s))
    sets = _sets(em)
    outs, refs = _run(em, sets, H.SCHEDULE, "nan")
    assert H.first_mismatch(outs, refs) == 0 and bool(torch.isnan(outs[0][0]).any())
    with pytest.raises(AssertionError, match=r"launch 0 of 6 .*NaN"):
        H.assert_sequence(outs, refs, "not yet written")
    # ... while identical re-launches see it on the first launch only: from the second on the location holds the same bits
    outs = [(em.launch(*sets[0]),) for _ in range(3)]
    assert H.first_mismatch(outs, refs, (0, 0, 0)) is None


def test_nan_words_are_nans_of_varying_payload():
    w = H.nan_words(4096)
    assert bool(torch.isnan(w.view(torch.float32)).all())
    assert bool((w[1:] != w[:-1]).all()) and w.unique().numel() > 2048
    assert not bool((w.view(torch.uint8).view(-1, 4) == 0).all(1).any())


def _allocation(w_bytes):
    buf = ((torch.arange(2 * H.GUARD + w_bytes, dtype=torch.int64) * 131 + 89) % 251).to(torch.uint8)
    buf[H.GUARD:H.GUARD + w_bytes] = H.nan_words(w_bytes // 4).view(torch.uint8)
    return buf


def test_scratch_mask_catches_a_single_stray_store():
    W, Wp = 4 * H.TAIL_BYTES, 3 * H.TAIL_BYTES
    before = _allocation(W)
    before[H.GUARD + Wp - H.TAIL_BYTES:H.GUARD + Wp] = 0  # the tail of the first W' bytes
    assert H.scratch_violations(before, before.clone(), Wp) == []
    ok = before.clone()
    ok[H.GUARD:H.GUARD + 4096] = 7  # stores inside the usable region are the launch's business
    assert H.scratch_violations(before, ok, Wp) == [] and H.scratch_violations(before, ok, Wp, written_bytes=4096) == []
    one = torch.tensor([0, 0, 128, 63], dtype=torch.uint8)  # the four bytes of 1.0f
    cases = {
        "the tail's first counter": (H.GUARD + Wp - H.TAIL_BYTES, "counter tail"),
        "the tail's last counter": (H.GUARD + Wp - 4, "counter tail"),
        "just past W'": (H.GUARD + Wp, "at or beyond workspace_bytes"),
        "the last word of W": (H.GUARD + W - 4, "at or beyond workspace_bytes"),
        "the guard before": (H.GUARD - 4, "BEFORE"),
        "the guard after": (H.GUARD + W, "AFTER"),
    }
    for name, (off, expect) in cases.items():
        after = before.clone()
        after[off:off + 4] = one
        v = H.scratch_violations(before, after, Wp)
        assert len(v) == 1 and expect in v[0], (name, v)
    after = before.clone()
    after[H.GUARD + 4096:H.GUARD + 4100] = one  # one word past the documented extent of the path taken
    assert H.scratch_violations(before, after, Wp) == []
    v = H.scratch_violations(before, after, Wp, written_bytes=4096)
    assert len(v) == 1 and "beyond the documented scratch extent" in v[0]


def test_expected_reduction_follows_the_documented_extents():
    M, N = 1000, 328
    slab, frag2, frag4 = H.slab_bytes(2, M, N), H.fragment_bytes(2, M, N, 256, 160), H.fragment_bytes(4, M, N, 256, 160)
    assert (slab, frag2, frag4) == (2624000, 12 * 256 * 160 * 4, 3 * 12 * 256 * 160 * 4)
    T = H.TAIL_BYTES
    assert H.expected_reduction(2, M, N, 256, 160, slab + T) == (2, "fixup", frag2)
    assert H.expected_reduction(2, M, N, 256, 160, slab + T - 4) == (1, "unsplit", 0)
    assert H.expected_reduction(2, M, N, 256, 160, slab + T, fixup_max=0) == (2, "slab", slab)
    s4 = H.slab_bytes(4, M, N)
    assert s4 < frag4  # four slices of this shape: the fragments need MORE room than the slabs
    assert H.expected_reduction(4, M, N, 256, 160, s4 + T) == (4, "slab", s4)
    assert H.expected_reduction(4, M, N, 256, 160, frag4 + T - 4) == (4, "slab", s4)
    assert H.expected_reduction(4, M, N, 256, 160, frag4 + T) == (4, "fixup", frag4)
    assert H.expected_reduction(4, M, N, 256, 160, s4 + T - 4) == (1, "unsplit", 0)
