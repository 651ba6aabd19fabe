"""CPU: the book-keeping of dpvo_amd.long_term -- RetrievalLog with a scripted
scorer and FrameCache with CPU tensors.  Every expectation is worked out by
hand from retrieval_dbow.py / image_cache.py of the reference."""
import pytest
import torch

from dpvo_amd.long_term import FrameCache, RetrievalLog


class Scripted:
    """insert_and_query answers from a table {n: (score, j)}; logs the calls."""

    def __init__(self, table):
        self.table, self.calls = table, []

    def insert_and_query(self, n, image):
        self.calls.append((n, image))
        return self.table.get(n, (0.0, 0))


def _feed(log, frames):
    for n in frames:
        log(f"img{n}", n)


def test_keyframe_shifts_the_waiting_frames():
    log = RetrievalLog(Scripted({}))
    _feed(log, [3, 4, 5, 6])
    log.keyframe(4)  # below k stays, k goes, above k moves down
    assert log.image_buffer == {3: "img3", 4: "img5", 5: "img6"}
    log.keyframe(9)  # above everything: nothing moves
    assert log.image_buffer == {3: "img3", 4: "img5", 5: "img6"}
    log.keyframe(0)  # below everything: all move
    assert log.image_buffer == {2: "img3", 3: "img5", 4: "img6"}


def test_save_up_to_scores_in_order_and_once():
    sc = Scripted({})
    log = RetrievalLog(sc)
    _feed(log, [0, 1, 2, 3])
    log.save_up_to(1)
    assert sc.calls == [(0, "img0"), (1, "img1")] and log.stored_indices == {0, 1}
    assert sorted(log.image_buffer) == [2, 3]
    log.save_up_to(1)  # nothing new
    assert len(sc.calls) == 2
    log.save_up_to(-1)
    assert len(sc.calls) == 2
    log(f"again", 1)  # a frame index that was stored before cannot be stored again
    with pytest.raises(RuntimeError):
        log.save_up_to(1)


def test_threshold_nms_and_repeat():
    table = {
        100: (0.01, 10),   # below the threshold 0.04: ignored
        120: (0.9, 30),    # (120-100)^2 + (30-10)^2 = 800 < 50^2: suppressed by the confirmed loop
        160: (0.9, 10),    # 60^2 + 0 = 3600 >= 2500: kept
        161: (0.9, 11),
        163: (0.9, 13),    # 161 -> 163 is not consecutive
        164: (0.9, 14),
        165: (0.9, 15),    # 163, 164, 165: three in a row -> the middle pair
    }
    sc = Scripted(table)
    log = RetrievalLog(sc)
    log.confirm_loop(100, 10)
    frames = [100, 120, 160, 161, 162, 163, 164, 165]
    _feed(log, frames)
    out = []
    for n in frames:  # one frame becomes final at a time, as in the tracker
        log.save_up_to(n)
        out.append(log.detect_loop(0.04, num_repeat=3))
    # 160, 161 and (162 scores 0) 163: found = [160, 161, 163] at 163 -> 1 + 163 - 160 = 4 != 3
    assert out == [None, None, None, None, None, None, None, (164, 14)]
    assert log.found == [(160, 10), (161, 11), (163, 13), (164, 14), (165, 15)]
    with pytest.raises(ValueError):
        log.confirm_loop(10, 100)


def test_repeat_one_and_j_zero():
    log = RetrievalLog(Scripted({7: (0.5, 0), 8: (0.5, 3)}))
    _feed(log, [7, 8])
    log.save_up_to(8)
    assert log.detect_loop(0.04, num_repeat=1) == (7, 1)  # j = 0 is returned as 1
    assert log.detect_loop(0.04, num_repeat=1) == (8, 3)
    assert log.detect_loop(0.04, num_repeat=1) is None
    log2 = RetrievalLog(Scripted({7: (0.5, 7)}))
    _feed(log2, [7])
    log2.save_up_to(7)
    with pytest.raises(ValueError):  # the scorer must answer an earlier frame
        log2.detect_loop(0.04)


def test_detect_loop_stops_at_the_first_hit_and_keeps_the_rest():
    log = RetrievalLog(Scripted({n: (0.5, n - 5) for n in range(10, 16)}))
    _feed(log, range(10, 16))
    log.save_up_to(15)
    assert log.detect_loop(0.04, num_repeat=3) == (11, 6)
    log.found.clear()  # what attempt_loop_closure does after a candidate
    assert log.detect_loop(0.04, num_repeat=3) == (14, 9)
    assert log.detect_loop(0.04, num_repeat=3) is None


def _img(n):
    return torch.full((3, 2, 2), n, dtype=torch.uint8)


def test_frame_cache_slots_recycling_and_eviction():
    cache = FrameCache(capacity=4, num_frames=16)
    for n in range(4):
        cache(_img(n), n)
    assert cache.slot_of_frame.shape == (16, 1) and cache.slot_of_frame.dtype == torch.int32
    assert cache.slot_of_frame[:5, 0].tolist() == [0, 1, 2, 3, -1]
    base = cache.slots.data_ptr()
    with pytest.raises(KeyError):  # nothing is final yet
        cache.load_frames([0, 1, 2])
    with pytest.raises(RuntimeError):  # full, and no final frame to evict
        cache(_img(4), 4)
    cache(_img(13), 3)  # the same frame index again: its slot is overwritten
    assert cache.slot_of_frame[3, 0] == 3 and cache.slots[3, 0, 0, 0] == 13

    cache.save_up_to(1)
    assert cache.load_frames([0, 1])[:, 0, 0, 0].tolist() == [0, 1]
    cache(_img(4), 4)  # evicts the oldest final frame, 0, and takes its slot
    assert cache.slot_of_frame[:5, 0].tolist() == [-1, 1, 2, 3, 0]
    assert 0 not in cache and 4 in cache
    with pytest.raises(KeyError):
        cache.load_frames([0])

    # frame 3 is dropped: 4 becomes 3, slot 3 is free again; the images stay where they are
    cache.keyframe(3)
    cache.shift_table(3)
    assert cache.slot_of_frame[:4, 0].tolist() == [-1, 1, 2, 0]
    assert cache.slots.data_ptr() == base and cache.slots[0, 0, 0, 0] == 4
    cache(_img(5), 4)
    assert cache.slot_of_frame[4, 0] == 3  # the recycled slot
    cache.save_up_to(4)
    assert cache.load_frames([2, 3, 4])[:, 0, 0, 0].tolist() == [2, 4, 5]
    cache(_img(6), 5)  # full again: frame 1 is the oldest final one now
    assert cache.slot_of_frame[1, 0] == -1 and cache.slot_of_frame[5, 0] == 1
    with pytest.raises(TypeError):
        cache(torch.zeros(3, 2, 2), 6)
    with pytest.raises(ValueError):
        FrameCache(capacity=2, num_frames=16)
