"""CPU-only: the host checks of the render-time entry points that take a `sample_major` argument (csrc/render_time.hip,
csrc/render_infer.hip), pinned by return code and by the WHOLE scanerf_last_error() text.  Every case is refused (or, for an
empty batch, accepted) before any launch, so no GPU is needed; where a later check is the target the pointers are small non-null
dummies that nothing dereferences.  The texts were taken from a library built before the unit was split (commit 2f39c6d)."""
import pytest

P = 64          # a non-null dummy pointer
T = 16          # a power-of-two table size
H3, F32, FOLDED = 8, 16, 32   # SCANERF_INFER_* of include/scanerf_hip.h


def _lib():
    import scanerf_amd  # noqa
    from scanerf_amd import _capi
    return _capi.lib()


# entry -> (its name in the error texts, pointer count, how to build the argument list from pointers and sizes)
def _sample_points(p, B, sm, **kw):
    return [*p, B, 8, kw.get("nb", 2), sm, None]


def _prepare_points(p, B, sm, **kw):
    return [*p, B, 8, kw.get("nb", 2), sm, None]


def _pts_inference(p, B, sm, **kw):
    return [*p, B, 8, kw.get("T", T), kw.get("nb", 2), sm, None]


def _bg(p, B, sm, **kw):
    return [*p[:4], 0, *p[4:], B, 8, kw.get("T", T), kw.get("nb", 2), sm, None]


def _accumulate(p, B, sm, **kw):
    return [*p, B, 8, sm, None]


def _inverse_z(p, B, sm, **kw):
    return [*p, 1.0, B, 8, kw.get("nb", 2), sm, None]


ENTRIES = {
    "scanerf_render_sample_points": ("sample_points", 13, _sample_points),
    "scanerf_prepare_points": ("prepare_points", 4, _prepare_points),
    "scanerf_pts_inference": ("pts_inference", 16, _pts_inference),
    "scanerf_pts_inference_tracing": ("pts_inference", 17, _pts_inference),
    "scanerf_bg_pts_inference_v2": ("bg_pts_inference_v2", 12, _bg),
    "scanerf_accumulate_color": ("accumulate_color", 8, _accumulate),
    "scanerf_render_inverse_z_sampling": ("inverse_z_sampling", 3, _inverse_z),
}
INFER = ("scanerf_pts_inference", "scanerf_pts_inference_tracing", "scanerf_bg_pts_inference_v2")
# the pointers the two foreground wrappers check themselves, before anything else: block_idxs / running_mask, intersections
OWN = {"scanerf_pts_inference": (4,), "scanerf_pts_inference_tracing": (4, 5)}


def _call(entry, ptrs, B, sm, **kw):
    lib = _lib()
    rc = getattr(lib, entry)(*ENTRIES[entry][2](ptrs, B, sm, **kw))
    return rc, lib.scanerf_last_error().decode()


def _ptrs(entry, value, own=None):
    """Every pointer of `entry` = value; with `own`, the pointers its wrapper checks itself (OWN) = own."""
    p = [value] * ENTRIES[entry][1]
    if own is not None:
        for k in OWN.get(entry, ()):
            p[k] = own
    return p


@pytest.mark.parametrize("entry", ENTRIES)
def test_layout_argument_is_checked(entry):
    name = ENTRIES[entry][0]
    assert _call(entry, _ptrs(entry, P), 32, 3) == (2, f"{name}: sample_major=3 (0, 1, or 2 with B a multiple of 32; B=32)")
    assert _call(entry, _ptrs(entry, P), 33, 2) == (2, f"{name}: sample_major=2 (0, 1, or 2 with B a multiple of 32; B=33)")
    # layout 1 takes any B: the next check answers
    assert _call(entry, _ptrs(entry, None, own=P), 33, 1) == (2, f"{name}: bad argument (null pointer or negative size)")


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_arrays_are_refused(entry):
    # (the foreground inference wrappers' own pointers are set: their check comes first and has its own text, below)
    name = ENTRIES[entry][0]
    assert _call(entry, _ptrs(entry, None, own=P), 32, 0) == (2, f"{name}: bad argument (null pointer or negative size)")
    for sm in (1, 2):
        assert _call(entry, _ptrs(entry, None, own=P), 32, sm) == (2, f"{name}: bad argument (null pointer or negative size)")


@pytest.mark.parametrize("entry", ENTRIES)
def test_empty_batch_is_a_no_op_before_the_null_check(entry):
    for sm in (0, 1, 2):
        assert _call(entry, _ptrs(entry, None, own=P), 0, sm)[0] == 0
    if entry not in OWN:
        return
    # with EVERY pointer null the wrapper's own check answers first, empty batch or not
    own = {"scanerf_pts_inference": "pts_inference: null block_idxs",
           "scanerf_pts_inference_tracing": "pts_inference_tracing: null running_mask / intersections"}[entry]
    assert _call(entry, _ptrs(entry, None), 0, 0) == (2, own)


def test_empty_batch_still_checks_the_layout_and_the_table_size():
    assert _call("scanerf_accumulate_color", _ptrs("scanerf_accumulate_color", None), 0, 3) == \
        (2, "accumulate_color: sample_major=3 (0, 1, or 2 with B a multiple of 32; B=0)")
    assert _call("scanerf_bg_pts_inference_v2", _ptrs("scanerf_bg_pts_inference_v2", None), 0, 0, T=12) == \
        (2, "bg_pts_inference_v2: T=12 must be a power of two")


def test_wrappers_own_null_pointer_messages():
    assert _call("scanerf_pts_inference", [P] * 4 + [None] + [P] * 11, 32, 0) == (2, "pts_inference: null block_idxs")
    for p45 in ((None, P), (P, None), (None, None)):
        ptrs = [P] * 4 + list(p45) + [P] * 11
        assert _call("scanerf_pts_inference_tracing", ptrs, 32, 0) == (2, "pts_inference_tracing: null running_mask / intersections")
    # ... which come before the layout check
    assert _call("scanerf_pts_inference", [None] * 16, 32, 3) == (2, "pts_inference: null block_idxs")


@pytest.mark.parametrize("entry", INFER)
def test_table_size_must_be_a_power_of_two(entry):
    name = ENTRIES[entry][0]
    assert _call(entry, _ptrs(entry, P), 32, 0, T=12) == (2, f"{name}: T=12 must be a power of two")
    assert _call(entry, _ptrs(entry, P), 32, 0, T=1) == (2, f"{name}: T=1 must be a power of two")
    # the layout is judged first
    assert _call(entry, _ptrs(entry, P), 32, 3, T=12) == (2, f"{name}: sample_major=3 (0, 1, or 2 with B a multiple of 32; B=32)")


@pytest.mark.parametrize("entry", INFER)
def test_folded_images_are_for_the_16_sample_tile_kernel(entry):
    name = ENTRIES[entry][0]
    text = f"{name}: SCANERF_INFER_FOLDED images are for the 16-sample-tile kernel only (nb <= 64, no SCANERF_INFER_H3 / _F32)"
    assert _call(entry, _ptrs(entry, P), 32, FOLDED | H3) == (2, text)
    assert _call(entry, _ptrs(entry, P), 32, FOLDED | F32) == (2, text)
    assert _call(entry, _ptrs(entry, P), 32, FOLDED, nb=65) == (2, text)
    # null pointers are judged before it
    assert _call(entry, _ptrs(entry, None, own=P), 32, FOLDED | H3) == (2, f"{name}: bad argument (null pointer or negative size)")


@pytest.mark.parametrize("entry", INFER)
def test_sample_major_arrays_need_the_chunk_kernel(entry):
    name = ENTRIES[entry][0]
    for sm in (1, 2):
        assert _call(entry, _ptrs(entry, P), 32, sm | F32) == (2, f"{name}: sample-major arrays need the chunk kernel")
        assert _call(entry, _ptrs(entry, P), 32, sm, nb=65) == (2, f"{name}: sample-major arrays need the chunk kernel")


def test_tracing_entry_needs_the_16_sample_tile_kernel_and_few_tiles():
    entry = "scanerf_pts_inference_tracing"
    text = "pts_inference_tracing: needs the 16-sample-tile kernel and nb <= 8 tiles (nb=%d); use prepare_points + pts_inference"
    for sm in (0, 1, 2, 4):   # default SCANERF_INFER_* bits; 4 = SCANERF_SKIP_UNSAMPLED
        assert _call(entry, _ptrs(entry, P), 32, sm, nb=9) == (2, text % 9)
    assert _call(entry, _ptrs(entry, P), 32, H3) == (2, text % 2)
    assert _call(entry, _ptrs(entry, P), 32, F32) == (2, text % 2)
    assert _call(entry, _ptrs(entry, P), 32, 0, nb=65) == (2, text % 65)
