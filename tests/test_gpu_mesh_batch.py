"""GPU: the batched mesh extraction (qsp_mesh_extract_batch / qsp_mesh_from_volumes / qsp_mesh_fetch_batch, csrc/mesh_extract.hpp)
gives, item by item, exactly what the single calls give: marching cubes against scikit-image's own output
(tests/golden/mc_lewiner_volumes.npz) and the CPU restatement (oracle/mc_lewiner_oracle.py), vertices (float64) and faces bit
for bit IN ORDER; decoded volumes against extract_mesh_from_code's on the same pipe, bit for bit.  Sizes: 12^3 (less than a scan
block of 2048 points), 13^3 (crosses one, no multiple of the 64-point tile), 9^3, 32^3 (whole scan blocks)."""
import os

import numpy as np
import pytest

from oracle import mc_lewiner_oracle as ml
from oracle import mc_oracle as mo
from tests.test_gpu_mesh import gpu_decoder  # noqa: F401  (the module's decoder fixture)
from tests.test_oracle_mesh import noise_volume, sphere_volume

pytestmark = pytest.mark.gpu


def extractor(dec, dim, code_len=64, method="lewiner"):
    from qsp_slam_amd.reconstruct.optimizer import MeshExtractor
    return MeshExtractor(dec, code_len=code_len, voxels_dim=dim, method=method)


def same_mesh(got, verts, faces):
    v, f = got
    return (v.dtype == np.float64 and f.dtype == np.int32 and v.shape == verts.shape and f.shape == faces.shape
            and np.array_equal(f, faces) and np.array_equal(v.view(np.uint64), np.ascontiguousarray(verts).view(np.uint64)))


def single(me, code):
    """extract_mesh_from_code, or None where it raises for an empty surface as scikit-image does"""
    try:
        return me.extract_mesh_from_code(code, return_volume=True)
    except (ValueError, RuntimeError):
        return None


def same_as_single(batch_item, single_item):
    if single_item is None or batch_item is None:
        return single_item is None and batch_item is None
    return (np.array_equal(batch_item["sdf_volume"].view(np.uint32), single_item["sdf_volume"].view(np.uint32))
            and same_mesh((batch_item.vertices, batch_item.faces), single_item.vertices, single_item.faces))


def smooth_volume(dim):
    g = np.linspace(-1, 1, dim, dtype=np.float32)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    return (np.sin(3 * x) * np.cos(2 * y) + 0.5 * np.sin(4 * z + x) - 0.1).astype(np.float32)


def batch_codes(n_extra=2):
    """the codes of tests/test_gpu_mesh.py::test_extract_mesh_from_code (dims 32 and 64) and small random ones"""
    codes = [(0.05 * np.random.default_rng(dim).standard_normal(64)).astype(np.float32) for dim in (32, 64)]
    rng = np.random.default_rng(5)          # (the first is test_lewiner_mesh_from_code_is_the_default's code)
    return codes + [(0.05 * rng.standard_normal(64)).astype(np.float32) for _ in range(n_extra)]


# ---- 1. marching cubes alone, against scikit-image's output -------------------------------------------------------------------
@pytest.mark.parametrize("names", [("decoder32_0", "decoder32_1", "decoder32_2"), ("noise12_0", "noise12_1")])
def test_volumes_equal_scikit_image(gpu_decoder, golden_dir, names):
    g = np.load(os.path.join(golden_dir, "mc_lewiner_volumes.npz"))
    vols = [g["vol_" + k] for k in names]
    out = extractor(gpu_decoder, vols[0].shape[0]).meshes_from_volumes(vols)
    assert len(out) == len(names)
    for k, got in zip(names, out):
        assert got is not None and same_mesh(got, g[k + "_verts"], g[k + "_faces"]), k


# ---- 2. items without a surface ------------------------------------------------------------------------------------------------
def test_empty_items_between_and_alone(gpu_decoder, golden_dir):
    from qsp_slam_amd import _lib
    g = np.load(os.path.join(golden_dir, "mc_lewiner_volumes.npz"))
    plus, minus = np.ones((12,) * 3, np.float32), np.full((12,) * 3, -1.0, np.float32)
    me = extractor(gpu_decoder, 12)
    out = me.meshes_from_volumes([g["vol_noise12_0"], plus, g["vol_noise12_1"], minus])
    assert out[1] is None and out[3] is None
    assert same_mesh(out[0], g["noise12_0_verts"], g["noise12_0_faces"])
    assert same_mesh(out[2], g["noise12_1_verts"], g["noise12_1_faces"])
    host = _lib.f32c(np.stack([g["vol_noise12_0"], plus, g["vol_noise12_1"], minus]).reshape(4, -1))
    nv, nf = np.full(4, -7, np.int64), np.full(4, -7, np.int64)
    _lib.check(_lib.lib().qsp_mesh_from_volumes(me.handle, 4, _lib.fptr(host), _lib.i64ptr(nv), _lib.i64ptr(nf)))
    assert list(nv) == [len(g["noise12_0_verts"]), 0, len(g["noise12_1_verts"]), 0]
    assert list(nf) == [len(g["noise12_0_faces"]), 0, len(g["noise12_1_faces"]), 0]
    assert me.meshes_from_volumes([plus]) == [None]
    assert me.meshes_from_volumes([minus]) == [None]


# ---- 3. other sizes and passes, against the restatement ----------------------------------------------------------------------
@pytest.mark.parametrize("dim", [9, 13])
def test_passes_equal_the_restatement(gpu_decoder, dim):
    vols = [sphere_volume(dim), noise_volume(dim, dim), smooth_volume(dim), noise_volume(dim, dim + 1), sphere_volume(dim, r=0.7)]
    me = extractor(gpu_decoder, dim)
    whole = me.meshes_from_volumes(vols)                 # one pass
    me.set_batch_limit(2)                                # passes of 2, 2 and 1
    parts = me.meshes_from_volumes(vols)
    for i, vol in enumerate(vols):
        ov, of = ml.convert_sdf_voxels_to_mesh(vol)
        assert len(of) > 0 and same_mesh(parts[i], ov, of), i
        assert same_mesh(whole[i], ov, of), i


# ---- 4. from codes, every pipe -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [13, 32])
@pytest.mark.parametrize("prec", ["f32", "fp16x2", "bf16x3"])
def test_batch_of_codes_equals_the_single_calls(gpu_decoder, prec, dim):
    codes = batch_codes()
    gpu_decoder.set_precision(prec)
    try:
        me = extractor(gpu_decoder, dim)
        out = me.extract_meshes_from_codes(codes, return_volumes=True)
        ref = [single(me, c) for c in codes]
        plain = me.extract_meshes_from_codes(np.stack(codes))          # (an array, no volumes)
    finally:
        gpu_decoder.set_precision("f32")
    assert len(out) == len(codes)
    for i in range(len(codes)):
        assert ref[i] is not None and same_as_single(out[i], ref[i]), (prec, dim, i)
        assert out[i]["sdf_volume"].shape == (dim,) * 3
        assert same_mesh((plain[i].vertices, plain[i].faces), ref[i].vertices, ref[i].faces)
        with pytest.raises(KeyError):
            plain[i]["sdf_volume"]
        if dim == 32 and prec == "f32":     # what tests/test_gpu_mesh.py::test_lewiner_mesh_from_code_is_the_default pins
            ov, of = ml.convert_sdf_voxels_to_mesh(out[i]["sdf_volume"])
            assert out[i].vertices.dtype == np.float64 and np.array_equal(out[i].vertices, ov) and np.array_equal(out[i].faces, of)
            assert len(of) > 100 and mo.signed_volume(ov, of) > 0


def many_codes(n, width=64):
    return list((0.05 * np.random.default_rng(100 + n).standard_normal((n, width))).astype(np.float32))


@pytest.mark.parametrize("prec", ["f32", "fp16x2", "bf16x3"])
def test_runs_of_tiles_that_cross_volumes_equal_the_single_calls(gpu_decoder, prec):
    """17 codes at 32^3 are 17 x 512 = 8704 tiles, more than the 4096 workgroups of a launch: every workgroup runs 3 consecutive
    tiles, and since 512 is no multiple of 3 most volume boundaries fall inside a run -- the workgroup folds the next code into
    its layer-0 / layer-4 biases between two tiles (with 4 codes every workgroup has one tile and never does).  Volumes bit for bit
    against the single calls."""
    codes = many_codes(17)
    gpu_decoder.set_precision(prec)
    try:
        me = extractor(gpu_decoder, 32)
        out = me.extract_meshes_from_codes(codes, return_volumes=True)
        ref = [single(me, c) for c in codes]
    finally:
        gpu_decoder.set_precision("f32")
    assert not any(np.array_equal(ref[0]["sdf_volume"], r["sdf_volume"]) for r in ref[1:])     # (the codes do differ)
    for i in range(len(codes)):
        assert ref[i] is not None and same_as_single(out[i], ref[i]), (prec, i)


@pytest.mark.parametrize("prec", ["f32", "fp16x2"])
def test_code_batches_in_several_passes(gpu_decoder, prec):
    """5 codes in passes of 2, 2 and 1: the later passes read their codes and write their volumes at an offset"""
    codes = many_codes(5)
    gpu_decoder.set_precision(prec)
    try:
        me = extractor(gpu_decoder, 13)
        me.set_batch_limit(2)
        out = me.extract_meshes_from_codes(codes, return_volumes=True)
        ref = [single(me, c) for c in codes]
    finally:
        gpu_decoder.set_precision("f32")
    for i in range(len(codes)):
        assert ref[i] is not None and same_as_single(out[i], ref[i]), (prec, i)


# ---- 5. the narrow decoder form ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n_codes", [(13, 4), (21, 29)])
def test_narrow_decoder_codes_equal_the_single_calls(golden_dir, dim, n_codes):
    """the 4 x 256 / code 32 decoder on the split-fp16 pipe (the NARROW tile).  21^3 with 29 codes: 29 x 145 = 4205 tiles in runs
    of 2, 145 odd -- runs cross volumes as in the test above."""
    from qsp_slam_amd import DeepSdfDecoder
    d = DeepSdfDecoder.from_npz(os.path.join(golden_dir, "decoder_4x256_c32.npz"))
    try:
        d.set_precision("fp16x2")
        codes = [c[:32].copy() for c in batch_codes()] if n_codes == 4 else many_codes(n_codes, 32)
        me = extractor(d, dim, code_len=32)
        out = me.extract_meshes_from_codes(codes, return_volumes=True)
        ref = [single(me, c) for c in codes]
        for i in range(len(codes)):
            assert ref[i] is not None and same_as_single(out[i], ref[i]), i
        assert d.range_fallbacks == 0
        del me
    finally:
        d.close()


# ---- 6. the fp16 range flag ----------------------------------------------------------------------------------------------------
def test_range_fallback_and_its_refusal(golden_dir, monkeypatch):
    from qsp_slam_amd import _lib
    from tests.test_gpu_split_precision import _scaled_decoder
    monkeypatch.delenv("QSP_PRECISION", raising=False)
    d = _scaled_decoder(golden_dir, 1, 6e5, rows=list(range(64)))    # activations of layer 1 beyond fp16's range
    try:
        codes = [np.zeros(64, np.float32)] + batch_codes()[2:]
        me = extractor(d, 13)
        d.set_precision("fp16x2")
        n0 = d.range_fallbacks
        ref = [single(me, c) for c in codes]
        n1 = d.range_fallbacks
        assert n1 == n0 + len(codes)                                 # every one of these codes leaves the range: each single call fell back
        out = me.extract_meshes_from_codes(codes, return_volumes=True)
        assert d.range_fallbacks == n1 + 1                           # the batch: one pass, counted once
        for i in range(len(codes)):
            assert same_as_single(out[i], ref[i]), i
        me.set_batch_limit(2)                                        # passes of 2 and 1: the later pass falls back too, each counted once
        out = me.extract_meshes_from_codes(codes, return_volumes=True)
        assert d.range_fallbacks == n1 + 3
        for i in range(len(codes)):
            assert same_as_single(out[i], ref[i]), i
        d.set_range_fallback(False)
        with pytest.raises(_lib.QspError) as e:
            me.extract_meshes_from_codes(codes)
        assert e.value.code == _lib.QSP_ERR_UNSUPPORTED
        d.set_range_fallback(True)
        del me
    finally:
        d.close()


# ---- 7. state and arguments ----------------------------------------------------------------------------------------------------
def test_single_and_batch_state_do_not_disturb_each_other(gpu_decoder):
    dim = 13
    codes = batch_codes()
    me = extractor(gpu_decoder, dim)
    a = single(me, codes[0])
    out = me.extract_meshes_from_codes(codes[1:3], return_volumes=True)
    # the single call's result is still the one qsp_mesh_fetch sees
    from qsp_slam_amd import _lib
    v32 = np.empty((len(a.vertices), 3), np.float32)
    f = np.empty((len(a.faces), 3), np.int32)
    _lib.check(_lib.lib().qsp_mesh_fetch(me.handle, _lib.fptr(v32), _lib.i32ptr(f), None))
    assert np.array_equal(f, a.faces)
    b = single(me, codes[0])
    assert same_as_single(a, b)
    # ... and the batch result the one qsp_mesh_fetch_batch sees
    tot_f = sum(len(o.faces) for o in out)
    fb = np.empty((tot_f, 3), np.int32)
    _lib.check(_lib.lib().qsp_mesh_fetch_batch(me.handle, None, None, _lib.i32ptr(fb), None))
    assert np.array_equal(fb, np.concatenate([o.faces for o in out]))
    for i, c in enumerate(codes[1:3]):
        assert same_as_single(out[i], single(me, c))


def test_scratch_is_reused_and_grows(gpu_decoder):
    dim = 13
    vols = [sphere_volume(dim), noise_volume(dim, 3), smooth_volume(dim), noise_volume(dim, 4), sphere_volume(dim, r=0.7),
            noise_volume(dim, 5), smooth_volume(dim) + np.float32(0.05)]
    want = [ml.convert_sdf_voxels_to_mesh(v) for v in vols]
    me = extractor(gpu_decoder, dim)
    for idx in ([0, 1, 2], [3], [4, 5, 6, 0, 1, 2, 3]):
        out = me.meshes_from_volumes([vols[i] for i in idx])
        for got, i in zip(out, idx):
            assert same_mesh(got, *want[i]), (idx, i)


def _single_c_abi(me, call, host):
    """a single call and its float32 fetch through the C ABI (whatever method the handle has selected)"""
    from qsp_slam_amd import _lib
    nv, nf = np.zeros(1, np.int64), np.zeros(1, np.int64)
    _lib.check(call(me.handle, _lib.fptr(host), _lib.i64ptr(nv), _lib.i64ptr(nf)))
    return _fetch_single_f32(me, int(nv[0]), int(nf[0]))


def _fetch_single_f32(me, nv, nf):
    from qsp_slam_amd import _lib
    v, f = np.empty((nv, 3), np.float32), np.empty((nf, 3), np.int32)
    _lib.check(_lib.lib().qsp_mesh_fetch(me.handle, _lib.fptr(v), _lib.i32ptr(f), None))
    return v, f


def test_table_single_call_between_a_batch_and_its_fetch(gpu_decoder):
    """the scratch is shared, the results are not: a table-method single call (flags, counts and block sums in the scratch the
    Lewiner batch just used) gives the oracle's mesh, and the batch's meshes are still there afterwards"""
    from qsp_slam_amd import _lib
    L = _lib.lib()
    dim = 13
    me = extractor(gpu_decoder, dim)
    out = me.extract_meshes_from_codes(batch_codes()[:3])
    assert all(o is not None and len(o.faces) > 0 for o in out)
    vol = noise_volume(dim, dim)
    ov, of = mo.marching_cubes(vol)
    _lib.check(L.qsp_mesh_extractor_set_method(me.handle, 1))
    try:
        v, f = _single_c_abi(me, L.qsp_mesh_from_volume, _lib.f32c(vol.reshape(-1)))
    finally:
        _lib.check(L.qsp_mesh_extractor_set_method(me.handle, 0))
    assert len(of) > 0 and v.shape == ov.shape and np.array_equal(f, of) and np.array_equal(v.view(np.uint32), ov.view(np.uint32))
    bv = np.empty((sum(len(o.vertices) for o in out), 3), np.float64)
    bf = np.empty((sum(len(o.faces) for o in out), 3), np.int32)
    _lib.check(L.qsp_mesh_fetch_batch(me.handle, None, _lib.dptr(bv), _lib.i32ptr(bf), None))
    assert same_mesh((bv, bf), np.concatenate([o.vertices for o in out]), np.concatenate([o.faces for o in out]))
    v2, f2 = _fetch_single_f32(me, len(ov), len(of))
    assert np.array_equal(f2, of) and np.array_equal(v2.view(np.uint32), ov.view(np.uint32))


def test_scratch_grows_between_two_single_calls(gpu_decoder):
    """single call, a batch of 7 volumes (the scratch grows from one volume to seven), the same single call again"""
    dim = 13
    vols = [sphere_volume(dim), noise_volume(dim, 3), smooth_volume(dim), noise_volume(dim, 4), sphere_volume(dim, r=0.7),
            noise_volume(dim, 5), smooth_volume(dim) + np.float32(0.05)]
    code = batch_codes()[0]
    me = extractor(gpu_decoder, dim)
    a = single(me, code)
    out = me.meshes_from_volumes(vols)
    b = single(me, code)
    assert a is not None and len(a.faces) > 0 and same_as_single(a, b)
    for i, vol in enumerate(vols):
        assert same_mesh(out[i], *ml.convert_sdf_voxels_to_mesh(vol)), i


def test_a_failed_single_call_leaves_nothing_to_fetch(golden_dir, monkeypatch):
    from qsp_slam_amd import _lib
    from tests.test_gpu_split_precision import _scaled_decoder
    L = _lib.lib()
    monkeypatch.delenv("QSP_PRECISION", raising=False)
    d = _scaled_decoder(golden_dir, 1, 6e5, rows=list(range(64)))    # activations of layer 1 beyond fp16's range
    try:
        me = extractor(d, 13)
        d.set_precision("fp16x2")
        code = _lib.f32c(np.zeros(64, np.float32))
        nv, nf = np.zeros(1, np.int64), np.zeros(1, np.int64)
        assert L.qsp_mesh_extract(me.handle, _lib.fptr(code), _lib.i64ptr(nv), _lib.i64ptr(nf)) == _lib.QSP_OK      # (falls back)
        assert L.qsp_mesh_fetch(me.handle, None, None, None) == _lib.QSP_OK
        d.set_range_fallback(False)
        assert L.qsp_mesh_extract(me.handle, _lib.fptr(code), _lib.i64ptr(nv), _lib.i64ptr(nf)) == _lib.QSP_ERR_UNSUPPORTED
        assert L.qsp_mesh_fetch(me.handle, None, None, None) == _lib.QSP_ERR_INVALID
        d.set_range_fallback(True)
        del me
    finally:
        d.close()


def test_table_method_is_not_batched(gpu_decoder):
    from qsp_slam_amd import _lib
    me = extractor(gpu_decoder, 9, method="table")
    for call in (lambda: me.meshes_from_volumes([sphere_volume(9)]), lambda: me.extract_meshes_from_codes(batch_codes()[:1])):
        with pytest.raises(_lib.QspError) as e:
            call()
        assert e.value.code == _lib.QSP_ERR_UNSUPPORTED and "method" in str(e.value)


def test_arguments(gpu_decoder):
    from qsp_slam_amd import _lib
    L = _lib.lib()
    me = extractor(gpu_decoder, 9)
    assert me.extract_meshes_from_codes([]) == [] and me.meshes_from_volumes([]) == []
    assert me.extract_meshes_from_codes(np.zeros((0, 64), np.float32)) == []
    with pytest.raises(ValueError):
        me.meshes_from_volumes([np.zeros((4, 4, 4), np.float32)])
    buf = np.zeros(2 * 9 ** 3, np.float32)
    nv, nf = np.zeros(2, np.int64), np.zeros(2, np.int64)
    p, pv, pf = _lib.fptr(buf), _lib.i64ptr(nv), _lib.i64ptr(nf)
    for fn in (L.qsp_mesh_extract_batch, L.qsp_mesh_from_volumes):
        assert fn(None, 1, p, pv, pf) == _lib.QSP_ERR_INVALID
        assert fn(me.handle, 1, None, pv, pf) == _lib.QSP_ERR_INVALID
        assert fn(me.handle, 1, p, None, pf) == _lib.QSP_ERR_INVALID
        assert fn(me.handle, 1, p, pv, None) == _lib.QSP_ERR_INVALID
        assert fn(me.handle, -1, p, pv, pf) == _lib.QSP_ERR_INVALID
        assert fn(me.handle, 0, p, pv, pf) == _lib.QSP_OK
    fresh = extractor(gpu_decoder, 9)
    assert L.qsp_mesh_fetch_batch(fresh.handle, None, None, None, None) == _lib.QSP_ERR_INVALID     # no batch yet
    assert L.qsp_mesh_fetch_batch(None, None, None, None, None) == _lib.QSP_ERR_INVALID
    for bad in (0, -1, 65):
        assert L.qsp_mesh_extractor_set_batch_limit(me.handle, bad) == _lib.QSP_ERR_INVALID
    assert L.qsp_mesh_extractor_set_batch_limit(None, 1) == _lib.QSP_ERR_INVALID
    assert L.qsp_mesh_extractor_set_batch_limit(me.handle, 64) == _lib.QSP_OK


# ---- 8. the pybind11 module ----------------------------------------------------------------------------------------------------
def test_pybind_equals_the_ctypes_mirror(gpu_decoder):
    from qsp_slam_amd import reconstruct_hip as rh
    codes = np.stack(batch_codes()[:3])
    ref = extractor(gpu_decoder, 13).extract_meshes_from_codes(codes)
    out = rh.MeshExtractor(gpu_decoder, 64, 13).extract_meshes_from_codes(codes)
    assert isinstance(out, list) and len(out) == 3
    for o, r in zip(out, ref):
        assert r is not None and same_mesh((o.vertices, o.faces), r.vertices, r.faces)
    assert rh.MeshExtractor(gpu_decoder, 64, 13).extract_meshes_from_codes(np.zeros((0, 64), np.float32)) == []
