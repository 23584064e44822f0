"""CPU: the matcher's yardstick (tests/match_ref.py) on hand-worked cases, the fd_brief_match symbol, and
the loud failure of fd.brief_match without a GPU (no CPU fallback)."""
import os

import numpy as np
import pytest

from match_ref import match_ref


def words(*vals):
    return np.array([[v] for v in vals], np.uint32)


def test_ref_tie_goes_to_lowest_index():
    # 8-bit descriptors. q = 00001111; t0 and t1 differ from it in one bit each, t2 in all eight.
    q = words(0b00001111)
    t = words(0b00001110, 0b00001101, 0b11110000)
    idx, dist, counts = match_ref(q, t, length=8)
    assert idx.tolist() == [[0]]             # distance 1 twice: the lower train index
    assert dist.tolist() == [[[1, 1]]]       # the second equals the best on a tie
    assert counts.tolist() == [1]
    # bits above `length` are not part of the distance: garbage there changes nothing
    idx2, dist2, _ = match_ref(words(0xABCD000F), words(0x1200000E, 0xFF00000D, 0x000000F0), length=8)
    assert idx2.tolist() == [[0]] and dist2.tolist() == [[[1, 1]]]


def test_ref_invalid_entries():
    # t0 equals q0 but is invalid: never a candidate. q1 is invalid: -1 / -1 / -1.
    q = words(0b1111, 0b0000)
    t = words(0b1111, 0b0111, 0b0011)
    idx, dist, counts = match_ref(q, t, q_valid=[[1, 0]], t_valid=[[0, 1, 1]], length=8)
    assert idx.tolist() == [[1, -1]]
    assert dist.tolist() == [[[1, 2], [-1, -1]]]
    assert counts.tolist() == [1]
    # counts cut the sets (flag bits 25..31 of a count word are ignored); slots past q_counts keep `fill`
    idx, dist, counts = match_ref(q, t, q_counts=[1 | (1 << 30)], t_counts=[1], length=8, fill=77)
    assert idx.tolist() == [[0, 77]] and dist.tolist() == [[[0, -1], [77, 77]]] and counts.tolist() == [1]


def test_ref_cross_check_rejection():
    # Both queries are nearest to the only train descriptor (q0 at distance 1, q1 at 0); its best query
    # is q1, so q0's match is rejected. The raw distances are written either way; without a second
    # candidate the ratio test is skipped.
    q = words(0b01, 0b11)
    t = words(0b11)
    idx, dist, counts = match_ref(q, t, length=8, cross_check=True, max_ratio=0.5)
    assert idx.tolist() == [[-1, 0]]
    assert dist.tolist() == [[[1, -1], [0, -1]]]
    assert counts.tolist() == [1]
    idx, _, counts = match_ref(q, t, length=8)
    assert idx.tolist() == [[0, 0]] and counts.tolist() == [2]
    # equidistant queries: the lower query index keeps the train descriptor
    idx, _, _ = match_ref(words(0b01, 0b10), words(0b11), length=8, cross_check=True)
    assert idx.tolist() == [[0, -1]]
    # d1 == max_ratio * d2 exactly (8 == 0.5 * 16) is rejected; max_distance rejects d1 above it
    q, t = words(0x00), words(0xFF, 0xFFFF)
    assert match_ref(q, t, length=32, max_ratio=0.5)[0].tolist() == [[-1]]
    assert match_ref(q, t, length=32, max_ratio=0.51)[0].tolist() == [[0]]
    assert match_ref(q, t, length=32, max_distance=7)[0].tolist() == [[-1]]
    assert match_ref(q, t, length=32, max_distance=8)[0].tolist() == [[0]]


def test_library_has_fd_brief_match():
    import feature_detector_amd as fd

    L = fd.load()
    assert hasattr(L, "fd_brief_match")
    assert L.fd_brief_match(None, 1, None, None, None, None, 0, None, None, None, 0, None, None, None, 0) != 0
    assert callable(fd.brief_match)


def test_no_device_error():
    import feature_detector_amd as fd

    if os.environ.get("HIP_VISIBLE_DEVICES") is None:
        try:
            import torch

            has_gpu = torch.cuda.is_available()
        except Exception:
            has_gpu = False
        if not has_gpu:
            with pytest.raises(fd.FdError):  # fails loudly, no CPU fallback
                fd.brief_match(np.zeros((4, 8), np.uint32), np.zeros((4, 8), np.uint32))
