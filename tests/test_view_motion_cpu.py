"""The pure functions of the kinematic clip viewer (phc_amd/view_motion.py): frame times, hold-last-frame, key selection, tile pairing."""
import numpy as np
import pytest


def test_frame_times_hold_each_clips_last_frame():
    from phc_amd import view_motion as vm
    lengths = [1.0, 0.25, 2.0]
    assert vm.num_frames(lengths, 30) == 61 and vm.num_frames(lengths, 30, frames=12) == 12 and vm.num_frames([1.0], 24) == 25
    t = vm.frame_times(lengths, 30, 0, 61)
    assert t.shape == (61, 3) and t[0].tolist() == [0.0, 0.0, 0.0]
    assert np.allclose(t[:, 2], np.arange(61) / 30)                                    # the longest clip: t = i / fps throughout
    assert np.allclose(t[:8, 1], np.arange(8) / 30) and (t[8:, 1] == 0.25).all()        # 0.25 s = 7.5 frames: held from frame 8 on, exactly
    assert (t[31:, 0] == 1.0).all() and t[30, 0] == 1.0
    # chunks continue where the last one stopped
    assert np.array_equal(np.concatenate([vm.frame_times(lengths, 30, 0, 25), vm.frame_times(lengths, 30, 25, 36)]), t)


def test_common_frames_of_a_compared_pair():
    from phc_amd import view_motion as vm
    m = vm.common_frames([1.0, 0.5], [0.5, 2.0], 10, 0, 12)
    assert m[:, 0].tolist() == [True] * 6 + [False] * 6 and m[:, 1].tolist() == [True] * 6 + [False] * 6
    assert vm.common_frames([1.0], [1.0], 10, 8, 4)[:, 0].tolist() == [True, True, True, False]


def test_key_selection():
    from phc_amd import view_motion as vm
    keys = ["a", "b", "c", "d"]
    assert vm.select_keys(keys, None, 1) == ["a"] and vm.select_keys(keys, [], 3) == ["a", "b", "c"] and vm.select_keys(keys, None, 9) == keys
    assert vm.select_keys(np.array(keys), ["d", "b"], 1) == ["d", "b"]
    with pytest.raises(ValueError, match="zz"):
        vm.select_keys(keys, ["a", "zz"])
    with pytest.raises(ValueError, match="replay.clips"):
        vm.select_keys(keys, None, 0)
    assert vm.match_keys(["b", "a"], ["a", "b", "x"]) == ["b", "a"]
    with pytest.raises(ValueError, match="compare.*c"):
        vm.match_keys(["a", "c"], ["a", "b"])


def test_tile_pairing():
    from phc_amd import view_motion as vm
    assert vm.tile_layout(1, False) == (1, 1, [(0, 0)])
    assert vm.tile_layout(4, False) == (4, 2, [(0, 0), (0, 1), (0, 2), (0, 3)])
    assert vm.tile_layout(5, False)[:2] == (5, 3)
    tiles, cols, src = vm.tile_layout(1, True)
    assert (tiles, cols, src) == (2, 2, [(0, 0), (1, 0)])
    tiles, cols, src = vm.tile_layout(3, True)
    assert tiles == 6 and cols % 2 == 0 and src == [(0, 0), (1, 0), (0, 1), (1, 1), (0, 2), (1, 2)]
    for k in range(1, 10):                                                              # a pair never wraps around a row
        tiles, cols, src = vm.tile_layout(k, True)
        assert all(src[v][1] == src[v + 1][1] and (v % cols) + 1 < cols for v in range(0, tiles, 2))
