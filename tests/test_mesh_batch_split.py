"""CPU: split_batch_meshes (qsp_slam_amd/reconstruct/optimizer.py) -- the per-item results of a batched mesh extraction from the
concatenated arrays qsp_mesh_fetch_batch returns."""
import numpy as np
import pytest

from qsp_slam_amd.reconstruct.optimizer import split_batch_meshes


def _arrays(nv, nf):
    verts = np.arange(3 * sum(nv), dtype=np.float64).reshape(-1, 3)
    faces = np.arange(3 * sum(nf), dtype=np.int32).reshape(-1, 3)
    return verts, faces


def test_items_own_consecutive_rows_and_an_empty_item_in_the_middle_is_none():
    nv, nf = [4, 0, 3, 5], [2, 0, 6, 1]
    verts, faces = _arrays(nv, nf)
    vols = np.arange(4 * 8, dtype=np.float32).reshape(4, 2, 2, 2)
    out = split_batch_meshes(nv, nf, verts, faces, vols)
    assert len(out) == 4 and out[1] is None
    v0 = f0 = 0
    for i in (0, 2, 3):
        v0, f0 = sum(nv[:i]), sum(nf[:i])
        v, f, vol = out[i]
        assert v.dtype == np.float64 and f.dtype == np.int32
        assert np.array_equal(v, verts[v0:v0 + nv[i]]) and np.array_equal(f, faces[f0:f0 + nf[i]])
        assert np.array_equal(vol, vols[i])
        assert not np.shares_memory(v, verts) and not np.shares_memory(f, faces) and not np.shares_memory(vol, vols)
    # without volumes the third entry is None
    assert split_batch_meshes(nv, nf, verts, faces)[0][2] is None


def test_empty_items_first_last_and_alone():
    nv, nf = [0, 2, 0], [0, 1, 0]
    verts, faces = _arrays(nv, nf)
    out = split_batch_meshes(nv, nf, verts, faces)
    assert out[0] is None and out[2] is None
    assert np.array_equal(out[1][0], verts) and np.array_equal(out[1][1], faces)
    assert split_batch_meshes([0], [0], np.empty((0, 3)), np.empty((0, 3), np.int32)) == [None]


def test_no_items():
    assert split_batch_meshes([], [], np.empty((0, 3)), np.empty((0, 3), np.int32)) == []
    assert split_batch_meshes(np.zeros(0, np.int64), np.zeros(0, np.int64), np.empty((0, 3)), np.empty((0, 3), np.int32),
                              np.empty((0, 2, 2, 2), np.float32)) == []


def test_counts_that_do_not_add_up_are_refused():
    verts, faces = _arrays([3], [2])
    with pytest.raises(ValueError):
        split_batch_meshes([2], [2], verts, faces)
    with pytest.raises(ValueError):
        split_batch_meshes([3], [1], verts, faces)
    with pytest.raises(ValueError):
        split_batch_meshes([3, 0], [2], verts, faces)
