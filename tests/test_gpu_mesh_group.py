"""GPU: mesh extraction over a decoder group (qsp_mesh_extractor_create_group / qsp_mesh_extract_batch_group,
csrc/mesh_extract.hpp; MeshExtractorGroup): n codes of several classes -> n meshes in one call, every volume of the one
grid-decode launch decoded with the parameters of its class (k_group_grid_decode*, csrc/sdf_kernels.hpp).  The bar is bit
identity, item by item, with extract_mesh_from_code on an extractor of that class's decoder alone: decoded volume, float64
vertices, faces, order -- on every pipe, with runs of tiles that cross volume and decoder boundaries, in several passes, on the
narrow tile, and (the documented exception) f32 bits for every class of a pass that one class made fall back."""
import ast
import os

import numpy as np
import pytest

from oracle import mc_lewiner_oracle as ml
from tests.test_gpu_decoder_group import _reset, _set_all, members  # noqa: F401  (the three classes of the decoder-group tests)
from tests.test_gpu_mesh_batch import many_codes, same_as_single, same_mesh, single, smooth_volume
from tests.test_oracle_mesh import noise_volume

pytestmark = pytest.mark.gpu


def extractor(dec, dim, code_len=64):
    from qsp_slam_amd.reconstruct.optimizer import MeshExtractor
    return MeshExtractor(dec, code_len=code_len, voxels_dim=dim)


def group_of(decs, dim, code_len=64):
    """a MeshExtractorGroup over decs (class id = position) and the per-class extractors it was made from"""
    from qsp_slam_amd.reconstruct.optimizer import MeshExtractorGroup
    ext = {c: extractor(d, dim, code_len) for c, d in enumerate(decs)}
    return MeshExtractorGroup(ext), ext


def singles(ext, codes, cls):
    return [single(ext[c], code) for code, c in zip(codes, cls)]


# ---- 1. mixed classes, every pipe ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "bf16x3", "fp16x2"])
def test_mixed_classes_equal_the_per_class_single_calls(members, prec):
    """13^3 = 2197 points = 35 tiles, the last one ragged; 7 codes of three classes, interleaved.  Item 2 is item 0's code under
    class 2 instead of class 0: another decoder, another volume."""
    cls = [0, 1, 2, 0, 1, 2, 1]
    codes = many_codes(7)
    codes[2] = codes[0].copy()
    _set_all(members, prec)
    try:
        mg, ext = group_of(members, 13)
        out = mg.extract_meshes_from_codes(codes, cls, return_volumes=True)
        ref = singles(ext, codes, cls)
        plain = mg.extract_meshes_from_codes(np.stack(codes), np.array(cls))          # (arrays, no volumes)
        mg.close()
    finally:
        _reset(members)
    assert len(out) == len(codes)
    for i in range(len(codes)):
        assert ref[i] is not None and same_as_single(out[i], ref[i]), (prec, i)
        assert same_mesh((plain[i].vertices, plain[i].faces), ref[i].vertices, ref[i].faces), (prec, i)
        with pytest.raises(KeyError):
            plain[i]["sdf_volume"]
    assert not np.array_equal(out[0]["sdf_volume"], out[2]["sdf_volume"])              # the class index is used
    assert not np.array_equal(out[0]["sdf_volume"], out[3]["sdf_volume"])              # (and so is the code)


# ---- 2. runs of tiles that cross volumes and decoders -------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "fp16x2"])
def test_runs_of_tiles_that_cross_volumes_and_decoders(members, prec):
    """21^3 = 145 tiles per volume (odd), 29 codes: 4205 tiles, more than the 4096 workgroups of a launch, so every workgroup
    runs 2 consecutive tiles and most volume boundaries fall inside a run.  Classes i % 3: every volume boundary is a decoder
    boundary -- the workgroup folds the next code with the next decoder's weights and (fp16x2) stages that decoder's constants
    again.  The same items sorted by class: the decoder changes twice in the whole launch, and a workgroup whose run crosses a
    volume boundary inside a class must NOT need the constants staged again to be right."""
    n = 29
    codes = many_codes(n)
    cls = [i % 3 for i in range(n)]
    order = sorted(range(n), key=lambda i: cls[i])                                     # (stable: class 0's items first)
    _set_all(members, prec)
    try:
        mg, ext = group_of(members, 21)
        ref = singles(ext, codes, cls)
        before = [d.range_fallbacks for d in members]
        mixed = mg.extract_meshes_from_codes(codes, cls, return_volumes=True)
        by_class = mg.extract_meshes_from_codes([codes[i] for i in order], [cls[i] for i in order], return_volumes=True)
        after = [d.range_fallbacks for d in members]
        mg.close()
    finally:
        _reset(members)
    assert [cls[i] for i in order] == [0] * 10 + [1] * 10 + [2] * 9
    for i in range(n):
        assert ref[i] is not None and same_as_single(mixed[i], ref[i]), (prec, "mixed", i)
    for k, i in enumerate(order):
        assert same_as_single(by_class[k], ref[i]), (prec, "by class", k, i)
    assert after == before, (prec, before, after)                                      # nothing left fp16's range


# ---- 3. passes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "fp16x2"])
def test_passes_read_codes_and_classes_at_an_offset(members, prec):
    """5 codes in passes of 2, 2 and 1: the later passes read their codes AND their class indices at an offset"""
    cls = [2, 0, 0, 1, 2]
    codes = many_codes(5)
    _set_all(members, prec)
    try:
        mg, ext = group_of(members, 13)
        whole = mg.extract_meshes_from_codes(codes, cls, return_volumes=True)
        mg.set_batch_limit(2)
        parts = mg.extract_meshes_from_codes(codes, cls, return_volumes=True)
        ref = singles(ext, codes, cls)
        mg.close()
    finally:
        _reset(members)
    for i in range(len(codes)):
        assert ref[i] is not None and same_as_single(parts[i], ref[i]), (prec, i)
        assert same_as_single(whole[i], parts[i]), (prec, i)


# ---- 4. narrow members ---------------------------------------------------------------------------------------------------------
def _narrow_pair(golden_dir, seed=11, eps=0.02):
    """decoder_4x256_c32.npz, and the same with every weight and bias multiplied by (1 + eps N(0, 1)), seeded"""
    from qsp_slam_amd import DeepSdfDecoder
    path = os.path.join(golden_dir, "decoder_4x256_c32.npz")
    z = np.load(path, allow_pickle=False)
    meta = ast.literal_eval(str(z["meta"]))
    rng = np.random.default_rng(seed)
    st = {k: (z[k] * (1.0 + eps * rng.standard_normal(z[k].shape))).astype(np.float32) for k in z.files if k != "meta"}
    return [DeepSdfDecoder.from_npz(path),
            DeepSdfDecoder.from_state_dict(st, latent_in=meta["latent_in"], code_len=meta["latent_size"])]


def test_narrow_members_equal_the_single_calls(golden_dir):
    """two 4 x 256 / code 32 decoders on the split-fp16 pipe: the NARROW tile, whose slab counts come from each member's own tables"""
    decs = _narrow_pair(golden_dir)
    try:
        for d in decs:
            d.set_precision("fp16x2")
        assert all(d.narrow_tile for d in decs)
        cls = [0, 1, 1, 0]
        codes = many_codes(4, 32)
        mg, ext = group_of(decs, 13, code_len=32)
        out = mg.extract_meshes_from_codes(codes, cls, return_volumes=True)
        ref = singles(ext, codes, cls)
        for i in range(len(codes)):
            assert ref[i] is not None and same_as_single(out[i], ref[i]), i
        assert not np.array_equal(ref[0]["sdf_volume"], single(ext[1], codes[0])["sdf_volume"])    # (the members do differ)
        assert [d.range_fallbacks for d in decs] == [0, 0]
        mg.close()
        del ext
    finally:
        for d in decs:
            d.close()


# ---- 5. a group of one ---------------------------------------------------------------------------------------------------------
def test_a_group_of_one_is_its_members_batch_call(members):
    from qsp_slam_amd.reconstruct.optimizer import MeshExtractorGroup
    codes = many_codes(3)
    me = extractor(members[2], 13)
    mg = MeshExtractorGroup({5: me})
    out = mg.extract_meshes_from_codes(codes, [5, 5, 5], return_volumes=True)
    ref = me.extract_meshes_from_codes(codes, return_volumes=True)
    mg.close()
    for i in range(len(codes)):
        assert ref[i] is not None and same_as_single(out[i], ref[i]), i


# ---- 6. volumes and state ------------------------------------------------------------------------------------------------------
def test_volumes_and_the_batch_state_on_a_group_extractor(members):
    from qsp_slam_amd import _lib
    dim = 13
    vols = [noise_volume(dim, dim), np.ones((dim,) * 3, np.float32), smooth_volume(dim)]
    mg, _ = group_of(members, dim)
    out = mg.meshes_from_volumes(vols)
    want = [ml.convert_sdf_voxels_to_mesh(vols[0]), None, ml.convert_sdf_voxels_to_mesh(vols[2])]
    assert out[1] is None
    for i in (0, 2):
        assert len(want[i][1]) > 0 and same_mesh(out[i], *want[i]), i
    bv = np.empty((len(want[0][0]) + len(want[2][0]), 3), np.float64)
    bf = np.empty((len(want[0][1]) + len(want[2][1]), 3), np.int32)
    _lib.check(_lib.lib().qsp_mesh_fetch_batch(mg.handle, None, _lib.dptr(bv), _lib.i32ptr(bf), None))
    assert same_mesh((bv, bf), np.concatenate([want[0][0], want[2][0]]), np.concatenate([want[0][1], want[2][1]]))
    mg.close()


# ---- 7. the fp16 range flag: every member's own ----------------------------------------------------------------------------------
def test_range_fallback_of_one_member_repeats_the_pass_for_all(golden_dir, monkeypatch):
    """member 0 plain, member 1 with layer-1 activations beyond fp16's range.  Member 1's tiles raise member 1's flag; the pass
    is repeated on the f32 pipe for both classes and counted once, on member 0 (include/qsp_hip.h, as a group refinement call
    counts its own).  Nothing is provoked on the device: the flag is an ordinary result of the kernel."""
    from qsp_slam_amd import DeepSdfDecoder, _lib
    from tests.test_gpu_mesh_batch import batch_codes
    from tests.test_gpu_split_precision import _scaled_decoder
    monkeypatch.delenv("QSP_PRECISION", raising=False)
    decs = [DeepSdfDecoder.from_npz(os.path.join(golden_dir, "decoder_8x512.npz")),
            _scaled_decoder(golden_dir, 1, 6e5, rows=list(range(64)))]
    try:
        cls = [0, 1, 0, 1]
        codes = [batch_codes()[2], np.zeros(64, np.float32), batch_codes()[3], batch_codes()[2]]
        mg, ext = group_of(decs, 13)
        ref_f32 = singles(ext, codes, cls)                               # every member on the f32 pipe
        for d in decs:
            d.set_precision("fp16x2")
        ref_h2 = singles(ext, codes, cls)                                # member 1's fall back one by one, member 0's stay on fp16x2
        assert not same_as_single(ref_h2[0], ref_f32[0])                 # (so the two pipes do differ for member 0)
        n0 = [d.range_fallbacks for d in decs]
        out = mg.extract_meshes_from_codes(codes, cls, return_volumes=True)
        n1 = [d.range_fallbacks for d in decs]
        assert n1 == [n0[0] + 1, n0[1]], (n0, n1)                        # one pass repeated: once, on member 0
        for i, c in enumerate(cls):
            assert same_as_single(out[i], ref_h2[i] if c == 1 else ref_f32[i]), i
        for d in decs:
            d.set_range_fallback(False)
        with pytest.raises(_lib.QspError) as e:
            mg.extract_meshes_from_codes(codes, cls)
        assert e.value.code == _lib.QSP_ERR_UNSUPPORTED
        assert _lib.lib().qsp_mesh_fetch_batch(mg.handle, None, None, None, None) == _lib.QSP_ERR_INVALID
        assert [d.range_fallbacks for d in decs] == n1
        for d in decs:
            d.set_range_fallback(True)
        again = mg.extract_meshes_from_codes(codes, cls, return_volumes=True)      # (no flag was left behind by the refused call)
        assert [d.range_fallbacks for d in decs] == [n1[0] + 1, n1[1]]
        assert all(same_as_single(a, b) for a, b in zip(again, out))
        mg.close()
        del ext
    finally:
        for d in decs:
            d.close()


# ---- 8. arguments through the C ABI --------------------------------------------------------------------------------------------
def test_arguments(members):
    import ctypes as C
    from qsp_slam_amd import _lib
    from qsp_slam_amd.reconstruct.optimizer import create_voxel_grid
    L = _lib.lib()
    dim = 9
    mg, ext = group_of(members, dim)
    codes = _lib.f32c(np.stack(many_codes(2)))
    cls = np.array([0, 2], np.int32)
    nv, nf = np.full(2, -7, np.int64), np.full(2, -7, np.int64)
    p, pc, pv, pf = _lib.fptr(codes), _lib.i32ptr(cls), _lib.i64ptr(nv), _lib.i64ptr(nf)
    fn = L.qsp_mesh_extract_batch_group
    assert fn(None, 2, p, pc, pv, pf) == _lib.QSP_ERR_INVALID
    assert fn(mg.handle, 2, None, pc, pv, pf) == _lib.QSP_ERR_INVALID
    assert fn(mg.handle, 2, p, None, pv, pf) == _lib.QSP_ERR_INVALID
    assert fn(mg.handle, 2, p, pc, None, pf) == _lib.QSP_ERR_INVALID
    assert fn(mg.handle, 2, p, pc, pv, None) == _lib.QSP_ERR_INVALID
    assert fn(mg.handle, -1, p, pc, pv, pf) == _lib.QSP_ERR_INVALID
    assert L.qsp_mesh_fetch_batch(mg.handle, None, None, None, None) == _lib.QSP_ERR_INVALID      # no batch yet
    assert fn(mg.handle, 0, p, pc, pv, pf) == _lib.QSP_OK and list(nv) == [-7, -7]                # touches nothing
    assert L.qsp_mesh_fetch_batch(mg.handle, None, None, None, None) == _lib.QSP_ERR_INVALID
    for bad in (-1, 3):
        assert fn(mg.handle, 2, p, _lib.i32ptr(np.array([0, bad], np.int32)), pv, pf) == _lib.QSP_ERR_INVALID
    assert mg.extract_meshes_from_codes([], []) == []
    # the group call on an extractor over one decoder, the calls without classes on one over a group
    assert fn(ext[0].handle, 2, p, pc, pv, pf) == _lib.QSP_ERR_INVALID
    assert L.qsp_mesh_extract_batch(mg.handle, 2, p, pv, pf) == _lib.QSP_ERR_INVALID
    assert "qsp_mesh_extract_batch_group" in L.qsp_last_error().decode()
    assert L.qsp_mesh_extract(mg.handle, p, pv, pf) == _lib.QSP_ERR_INVALID
    assert "qsp_mesh_extract_batch_group" in L.qsp_last_error().decode()
    # creation
    pts = _lib.f32c(create_voxel_grid(dim))
    h = C.c_void_p()
    assert L.qsp_mesh_extractor_create_group(None, dim, _lib.fptr(pts), C.byref(h)) == _lib.QSP_ERR_INVALID
    assert L.qsp_mesh_extractor_create_group(mg.group.handle, dim, None, C.byref(h)) == _lib.QSP_ERR_INVALID
    assert L.qsp_mesh_extractor_create_group(mg.group.handle, dim, _lib.fptr(pts), None) == _lib.QSP_ERR_INVALID
    assert L.qsp_mesh_extractor_create_group(mg.group.handle, 1, _lib.fptr(pts), C.byref(h)) == _lib.QSP_ERR_UNSUPPORTED
    # method 1 is not batched, set_method / set_batch_limit work as on any extractor
    assert fn(mg.handle, 2, p, pc, pv, pf) == _lib.QSP_OK and nv.min() > 0 and nf.min() > 0
    _lib.check(L.qsp_mesh_extractor_set_method(mg.handle, 1))
    assert fn(mg.handle, 2, p, pc, pv, pf) == _lib.QSP_ERR_UNSUPPORTED
    _lib.check(L.qsp_mesh_extractor_set_method(mg.handle, 0))
    assert L.qsp_mesh_extractor_set_batch_limit(mg.handle, 65) == _lib.QSP_ERR_INVALID
    assert L.qsp_mesh_extractor_set_batch_limit(mg.handle, 1) == _lib.QSP_OK
    # a member whose options changed after creation: refused at the next call, as by every group entry point
    try:
        members[1].set_precision("bf16x3")
        assert fn(mg.handle, 2, p, pc, pv, pf) == _lib.QSP_ERR_UNSUPPORTED
    finally:
        _reset(members)
    assert fn(mg.handle, 2, p, pc, pv, pf) == _lib.QSP_OK
    mg.close()


# ---- 9. meshes with the refinement results ---------------------------------------------------------------------------------------
def _same_refinement(a, b):
    return (a.is_good == b.is_good and a.kept_flip == b.kept_flip and a.loss == b.loss and np.array_equal(a.losses, b.losses)
            and (not a.is_good or (np.array_equal(a.t_cam_obj, b.t_cam_obj) and np.array_equal(a.code, b.code))))


def _check_meshes(res, plain, mesh_of):
    for i, (r, q) in enumerate(zip(res, plain)):
        assert _same_refinement(r, q), i
        want = single(mesh_of(i), r.code) if r.is_good else None
        if want is None:
            assert r.vertices is None and r.faces is None, i
        else:
            assert same_mesh((r.vertices, r.faces), want.vertices, want.faces), i


def test_refine_detections_hands_back_the_meshes(members):
    """the detections of tests/test_gpu_decoder_group.py::test_refine_detections_by_class_equals_per_class_calls: three classes
    in the group, detections of classes 10 and 12"""
    from qsp_slam_amd import synth
    from qsp_slam_amd.reconstruct.optimizer import MeshExtractorGroup, OptimizerGroup
    from tests.test_gpu_decoder_group import _det_opt
    opts = {10 + c: _det_opt(d) for c, d in enumerate(members)}
    ext = {10 + c: extractor(d, 13) for c, d in enumerate(members)}
    dets = synth.make_detections(31, 6, 500, n_fg=96, n_bg=40, n_kf=2)
    dets[3]["found_good_orientation"] = True
    cids = [10, 12, 12, 10, 12, 10]
    for d, c in zip(dets, cids):
        d["class_id"] = c
    og = OptimizerGroup(opts)
    mg = MeshExtractorGroup(ext, decoder_group=og.group)                 # (the optimizers' decoder group serves both)
    plain = og.refine_detections(dets, flip_sample_num=4)
    res = og.refine_detections(dets, flip_sample_num=4, mesh_extractors=mg)
    assert any(r.is_good for r in res)
    assert all("vertices" not in q and "faces" not in q for q in plain)
    _check_meshes(res, plain, lambda i: ext[cids[i]])
    mg.close()
    og.close()
    # the single-class optimizer with a plain MeshExtractor
    idx = [i for i, c in enumerate(cids) if c == 12]
    mine = [dets[i] for i in idx]
    plain = opts[12].refine_detections(mine, flip_sample_num=4)
    res = opts[12].refine_detections(mine, flip_sample_num=4, mesh_extractor=ext[12])
    assert any(r.is_good for r in res)
    _check_meshes(res, plain, lambda i: ext[12])
