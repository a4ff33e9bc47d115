"""eval.py on prescribed predictions, or with its real forward recorded: started by tests/test_eval_report_gpu.py as a fresh child process.

    python tests/eval_driver.py --prescribed split.npz [--clip-range LO HI] [eval.py's arguments ...]
    python tests/eval_driver.py --record masks.npz [eval.py's arguments ...]

--prescribed replaces, before eval.main runs, gdkvm_amd.data.build_dataset with a dataset read from the .npz (tests/eval_fixture.
as_dataset_arrays: the uint8 frames carry the prescribed prediction's class index as the pixel value of every channel; `spacing` may be
missing: a split without pixel spacings) and gdkvm_amd.pipeline.SegmentRunner with a runner that decodes the class index from the frames the
prefetcher hands it, builds one-hot fp32 logits and returns ops.argmax_dice of them and the target -- masks and counts come from the product's
kernel, and everything behind the forward is eval.py as it stands, on the real DataLoader and DevicePrefetcher.  --clip-range replaces
gdkvm_amd.distributed.shard_range, so that this one process evaluates the clips LO .. HI - 1 as a rank of a larger job would.
--record keeps the real SegmentRunner and writes a copy of every batch's predicted masks, in order, to the .npz when eval.main returns."""
import argparse
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

    class PrescribedClips(torch.utils.data.Dataset):
        T = int(arrays["frames"].shape[1])

        def __len__(self):
            return int(arrays["frames"].shape[0])

        def __getitem__(self, i):
            return torch.from_numpy(arrays["frames"][i]), torch.from_numpy(arrays["target"][i])

        def spacing_um(self, i):
            return (int(arrays["spacing"][i][0]), int(arrays["spacing"][i][1])) if "spacing" in arrays else None

        def length(self, i):
            return int(arrays["lengths"][i])

        def file_ef(self, i):
            v = float(arrays["file_ef"][i])
            return None if np.isnan(v) else v

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
                raise RuntimeError(f"eval_driver: a frame byte of {int(idx.max())} is no class of {self.ncls}")
            logits = torch.nn.functional.one_hot(idx, self.ncls).permute(0, 1, 4, 2, 3).reshape(B * T, self.ncls, H, W).to(torch.float32).contiguous()
            mask, counts = ops.argmax_dice(logits, target.reshape(B * T, H, W).contiguous())
            self.seen[tuple(frames.shape)] = self.seen.get(tuple(frames.shape), 0) + 1
            if self.seen[tuple(frames.shape)] >= 2:
                self.replays += 1
            else:
                self.eager_calls += 1
            return Result((mask.reshape(B, T, H, W), counts.reshape(B, T, self.ncls, 3)))

    D.build_dataset = lambda cfg, split="train", n_synthetic=256, as_uint8=False: PrescribedClips()
    P.SegmentRunner = PrescribedRunner


def clip_range(lo, hi):
    import gdkvm_amd.distributed as X

    def fixed(n, world, rank):
        if not 0 <= lo <= hi <= n:
            raise ValueError(f"eval_driver: clips {lo}..{hi} of {n}")
        return lo, hi

    X.shard_range = fixed


def record():
    """Wraps the real SegmentRunner.submit: every get() also leaves a host copy of its masks in the returned list."""
    import gdkvm_amd.pipeline as P

    masks, submit = [], P.SegmentRunner.submit

    def recording(self, frames, target=None):
        pending = submit(self, frames, target)
        get = pending.get

        def keep():
            out = get()
            masks.append(out[0].clone().cpu())
            return out

        pending.get = keep
        return pending

    P.SegmentRunner.submit = recording
    return masks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prescribed", default="")
    ap.add_argument("--clip-range", nargs=2, type=int, default=None)
    ap.add_argument("--record", default="")
    args, rest = ap.parse_known_args()
    if args.prescribed:
        prescribed(args.prescribed)
    if args.clip_range:
        clip_range(*args.clip_range)
    masks = record() if args.record else None
    import eval as E
    E.main(rest)
    if args.record:
        np.savez(args.record, masks=torch.cat(masks).numpy(), batches=np.asarray([m.shape[0] for m in masks]))


if __name__ == "__main__":
    main()
