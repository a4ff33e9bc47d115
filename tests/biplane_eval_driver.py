"""eval.py on prescribed predictions of a split whose clips are the views of patients: started by tests/test_biplane_eval_gpu.py as a fresh
child process.

    python tests/biplane_eval_driver.py --prescribed split.npz [--clip-range LO HI] [--and-without] [eval.py's arguments ...]

As tests/eval_driver.py's prescribed mode: before eval.main runs, gdkvm_amd.data.build_dataset is replaced with a dataset read from the .npz
(tests/biplane_eval_fixture.as_dataset_arrays: the uint8 frames carry the prescribed prediction's class index as the pixel value of every
channel; `spacing` may be missing) and gdkvm_amd.pipeline.SegmentRunner with a runner that decodes the class index and returns
ops.argmax_dice of one-hot logits and the target -- everything behind the forward is eval.py as it stands.  The dataset also answers
patient(i), view(i) and info(i) (`patients`, `views`: arrays of names; `info`: one JSON text per clip, "null" for none), which is what
data.lv_biplane needs.  --clip-range replaces gdkvm_amd.distributed.shard_range, so that this one process evaluates the clips LO .. HI - 1 as
a rank of a larger job would.  --and-without runs eval.main a second time with data.lv_biplane=false appended: a second JSON line, the same
run's report without the key."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch


def prescribed(path):
    import gdkvm_amd.data as D
    import gdkvm_amd.pipeline as P
    from gdkvm_amd import ops

    with np.load(path) as z:
        arrays = {k: z[k] for k in z.files}
    infos = [json.loads(str(s)) for s in arrays["info"]]

    class PatientClips(torch.utils.data.Dataset):
        T = int(arrays["frames"].shape[1])

        def __len__(self):
            return int(arrays["frames"].shape[0])

        def __getitem__(self, i):
            return torch.from_numpy(arrays["frames"][i]), torch.from_numpy(arrays["target"][i])

        def spacing_um(self, i):
            return (int(arrays["spacing"][i][0]), int(arrays["spacing"][i][1])) if "spacing" in arrays else None

        def patient(self, i):
            return str(arrays["patients"][i])

        def view(self, i):
            return str(arrays["views"][i])

        def info(self, i):
            return infos[i]

    class Result:
        def __init__(self, out):
            self.out = out

        def get(self):
            return self.out

    class PrescribedRunner:
        """SegmentRunner's interface: submit(frames [B, T, 3, H, W] in [0, 1], target uint8 [B, T, H, W]) -> an object whose get() gives (mask
        uint8 [B, T, H, W], counts int32 [B, T, ncls, 3]); a batch shape counts as a replay from its second batch on, as the real runner's."""

        def __init__(self, model, **kw):
            self.ncls, self.replays, self.eager_calls, self.seen = int(model.cfg.num_classes), 0, 0, {}

        def submit(self, frames, target=None):
            B, T, _, H, W = frames.shape
            idx = torch.round(frames[:, :, 0].to(torch.float32) * 255.0).to(torch.int64)
            if int(idx.max()) >= self.ncls:
                raise RuntimeError(f"biplane_eval_driver: a frame byte of {int(idx.max())} is no class of {self.ncls}")
            logits = torch.nn.functional.one_hot(idx, self.ncls).permute(0, 1, 4, 2, 3).reshape(B * T, self.ncls, H, W).to(torch.float32).contiguous()
            mask, counts = ops.argmax_dice(logits, target.reshape(B * T, H, W).contiguous())
            self.seen[tuple(frames.shape)] = self.seen.get(tuple(frames.shape), 0) + 1
            if self.seen[tuple(frames.shape)] >= 2:
                self.replays += 1
            else:
                self.eager_calls += 1
            return Result((mask.reshape(B, T, H, W), counts.reshape(B, T, self.ncls, 3)))

    D.build_dataset = lambda cfg, split="train", n_synthetic=256, as_uint8=False: PatientClips()
    P.SegmentRunner = PrescribedRunner


def clip_range(lo, hi):
    import gdkvm_amd.distributed as X

    def fixed(n, world, rank):
        if not 0 <= lo <= hi <= n:
            raise ValueError(f"biplane_eval_driver: clips {lo}..{hi} of {n}")
        return lo, hi

    X.shard_range = fixed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prescribed", required=True)
    ap.add_argument("--clip-range", nargs=2, type=int, default=None)
    ap.add_argument("--and-without", action="store_true")
    args, rest = ap.parse_known_args()
    prescribed(args.prescribed)
    if args.clip_range:
        clip_range(*args.clip_range)
    import eval as E
    E.main(rest)
    if args.and_without:
        E.main(rest + ["data.lv_biplane=false"])


if __name__ == "__main__":
    main()
