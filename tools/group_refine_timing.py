"""Decoder groups: one mixed-class refinement batch against the per-class batches it replaces.

Three 8 x 512 classes (decoder_8x512 weights, the same with use_tanh, and a seeded perturbation), each with 4 objects x 4 yaw
flips and C2-sized observations (2 k surface points, 256 foreground + 200 background rays), 5 Gauss-Newton iterations on the
split-fp16 pipe with render screening (bench.py's default pipe).  Timed with qsp_refine_batch_profile (HIP events on the
library's stream, first launch -> last kernel), median of --reps runs of each:
  mixed    -- the 12 objects of the three classes in one batch over the group;
  single   -- the same 12 objects in one batch of ONE decoder (the cost the mixed batch is compared against);
  per-class sum -- the three one-class batches of 4 objects each that the mixed batch replaces.
Prints one JSON line."""
import argparse
import ast
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import bench
    from qsp_slam_amd import DecoderGroup, DeepSdfDecoder, synth
    from qsp_slam_amd.reconstruct.optimizer import Optimizer, RefineBatch, _flip_rotation, _joint_cfg
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--precision", default="fp16x2")
    ap.add_argument("--screening", type=float, default=0.01)
    args = ap.parse_args()
    path = os.path.join(ROOT, "tests", "golden", "decoder_8x512.npz")
    z = np.load(path, allow_pickle=False)
    meta = ast.literal_eval(str(z["meta"]))
    rng = np.random.default_rng(5)
    pert = {k: (z[k] * (1.0 + 0.02 * rng.standard_normal(z[k].shape))).astype(np.float32) for k in z.files if k != "meta"}
    decs = [DeepSdfDecoder.from_npz(path), DeepSdfDecoder.from_npz(path),
            DeepSdfDecoder.from_state_dict(pert, latent_in=meta["latent_in"], code_len=meta["latent_size"])]
    decs[1].set_use_tanh(True)
    for d in decs:
        d.set_precision(args.precision)
        if args.screening and args.precision == "fp16x2":
            d.set_render_screening(args.screening)
    cfg = _joint_cfg(Optimizer(decs[0], bench.joint_cfg(5)))
    objs = synth.make_object_views(7, 12, 2000, n_fg=256, n_bg=200)
    cls = np.array([i % 3 for i in range(12)], np.int32)

    def batch_ms(target, sel, obj_class=None):
        ob = [objs[i] for i in sel]
        hyp = np.repeat(np.arange(len(ob)), 4)
        T0 = np.stack([_flip_rotation(o["t_cam_obj"], k, 2 * np.pi / 4) for o in ob for k in range(4)])
        b = RefineBatch(target, cfg, [o["pts"] for o in ob], [o["rays"] for o in ob], [o["depth"] for o in ob], hyp,
                        obj_class=obj_class)
        b.profile(True)
        ms = []
        for _ in range(args.reps + 1):
            b.set_state(T0, None)
            b.run(0)
            ms.append(b.profile(True).ms_total)
        b.close()
        return float(np.median(ms[1:]))

    g = DecoderGroup(decs)
    mixed = batch_ms(g, range(12), cls)
    single = batch_ms(decs[0], range(12))
    per_class = [batch_ms(decs[c], np.nonzero(cls == c)[0]) for c in range(3)]
    g.close()
    print(json.dumps(dict(case="3 classes x 4 objects x 4 flips, 2k points, 256 fg + 200 bg rays, 5 iterations",
                          precision=args.precision, screening=args.screening, reps=args.reps,
                          ms_mixed=round(mixed, 3), ms_single_decoder_same_12=round(single, 3),
                          ms_per_class=[round(x, 3) for x in per_class], ms_per_class_sum=round(sum(per_class), 3),
                          mixed_over_single=round(mixed / single, 3), target_mixed_over_single=1.3)))
    for d in decs:
        d.close()


if __name__ == "__main__":
    main()
