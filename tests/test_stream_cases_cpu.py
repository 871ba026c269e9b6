"""The registry of tests/stream_cases.py, checked without a GPU: every export of include/scanerf_hip.h that takes a stream is claimed by
a case, and the two seeds of every case are interchangeable -- equal keys, shapes and dtypes, every floating-point input different (a
stale read is visible), every integer input of either seed inside the ranges the case states for its own sizes (a stale read is a wrong
answer, never an out-of-range index).  The GPU half (tests/test_gpu_stream_contract.py) rests on the second property."""
import pytest
import torch

import stream_cases as SC


def test_header_parse_agrees_with_the_prototype_table():
    """The parse finds the exports whose last parameter is the stream: exactly those of _capi.PROTOTYPES that end in a pointer and are
    no size / query function."""
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi
    names = SC.stream_entries()
    assert len(names) == len(set(names)) and len(names) >= 82, len(names)
    assert set(names) <= set(_capi.PROTOTYPES)
    for n in names:
        assert _capi.PROTOTYPES[n][1].endswith("P"), n
    for n, (ret, args, _) in _capi.PROTOTYPES.items():
        if n not in names:
            assert ret != "I" or not args.endswith("P") or n == "scanerf_icache_sweep", f"{n} looks like a launch the parse missed"


def test_every_stream_taking_export_is_claimed_by_a_case():
    names = set(SC.stream_entries())
    claimed = set().union(*(c.entries for c in SC.CASES))
    assert not claimed - names, f"cases claim names the header lacks: {sorted(claimed - names)}"
    assert not set(SC.EXEMPT) - names, sorted(set(SC.EXEMPT) - names)
    for name, why in SC.EXEMPT.items():
        assert isinstance(why, str) and why.count(".") <= 1 and len(why) > 20, (name, why)
    missing = names - claimed - set(SC.EXEMPT)
    assert not missing, f"no case claims {sorted(missing)}"
    assert not claimed & set(SC.EXEMPT), "an exempt entry is claimed as well"


def test_optional_entries_are_the_optional_prototypes():
    import scanerf_amd  # noqa: F401
    from scanerf_amd import _capi
    for c in SC.CASES:
        for e in c.entries:
            assert (e in c.optional) == (not _capi.PROTOTYPES[e][2]), (c.name, e)


def test_the_two_inexact_cases_are_the_float_atomic_table_gradients():
    inexact = {c.name: c for c in SC.CASES if not c.exact}
    assert set().union(*(c.entries for c in inexact.values())) == {"scanerf_embedding_bg_backward", "scanerf_embedding_backward"}
    for c in inexact.values():
        assert c.reference is not None and c.compare is not None


def _in_range(t, rng):
    if isinstance(rng, list):
        assert t.shape[-1] == len(rng)
        return all(_in_range(t[..., k], r) for k, r in enumerate(rng))
    lo, hi = rng
    return int(t.min()) >= lo and int(t.max()) < hi


@pytest.mark.parametrize("c", SC.CASES, ids=lambda c: c.name)
def test_seeds_are_interchangeable(c):
    a, b = c.build(1), c.build(2)
    assert list(a) == list(b)
    ints = set()
    for k in a:
        x, y = a[k], b[k]
        assert isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor) and not x.is_cuda, k
        assert x.shape == y.shape and x.dtype == y.dtype, (k, x.shape, y.shape, x.dtype, y.dtype)
        if x.dtype.is_floating_point:
            assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(y).all()), k
            assert not torch.equal(x, y), f"{c.name}: the float input {k} is the same in both seeds"
        elif x.dtype != torch.bool:
            ints.add(k)
            assert k in c.int_ranges, f"{c.name}: the integer input {k} has no stated range"
            assert _in_range(x, c.int_ranges[k]) and _in_range(y, c.int_ranges[k]), (c.name, k)
    assert ints == set(c.int_ranges), f"{c.name}: ranges for {sorted(set(c.int_ranges) - ints)} name no integer input"
    # a second build of a seed gives the same tensors: the registry is deterministic
    for k, v in c.build(1).items():
        assert torch.equal(v, a[k]), k
