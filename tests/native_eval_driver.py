"""eval.py on prescribed predictions of an npy_clips tree with native targets: started by tests/test_native_eval_gpu.py as a fresh child
process.

    python tests/native_eval_driver.py [--clip-range LO HI] [--and-without] [eval.py's arguments ...]

The dataset is the real one (gdkvm_amd.data.NpzClips over the tree tests/native_eval_fixture.write_split wrote: the uint8 frames carry the
prescribed prediction's class index as the pixel value of every channel).  Before eval.main runs, gdkvm_amd.pipeline.SegmentRunner is
replaced with a runner that decodes the class index and returns ops.argmax_dice of one-hot logits and the target -- everything behind the
forward is eval.py as it stands.  --clip-range replaces gdkvm_amd.distributed.shard_range, so that this one process evaluates the clips
LO .. HI - 1 as a rank of a larger job would.  --and-without runs eval.main a second time with data.native_eval=false appended: a second
JSON line, the same run's report without the key."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch


def prescribed():
    import gdkvm_amd.pipeline as P
    from gdkvm_amd import ops

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
                raise RuntimeError(f"native_eval_driver: a frame byte of {int(idx.max())} is no class of {self.ncls}")
            logits = torch.nn.functional.one_hot(idx, self.ncls).permute(0, 1, 4, 2, 3).reshape(B * T, self.ncls, H, W).to(torch.float32).contiguous()
            mask, counts = ops.argmax_dice(logits, target.reshape(B * T, H, W).contiguous())
            self.seen[tuple(frames.shape)] = self.seen.get(tuple(frames.shape), 0) + 1
            if self.seen[tuple(frames.shape)] >= 2:
                self.replays += 1
            else:
                self.eager_calls += 1
            return Result((mask.reshape(B, T, H, W), counts.reshape(B, T, self.ncls, 3)))

    P.SegmentRunner = PrescribedRunner


def clip_range(lo, hi):
    import gdkvm_amd.distributed as X

    def fixed(n, world, rank):
        if not 0 <= lo <= hi <= n:
            raise ValueError(f"native_eval_driver: clips {lo}..{hi} of {n}")
        return lo, hi

    X.shard_range = fixed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clip-range", nargs=2, type=int, default=None)
    ap.add_argument("--and-without", action="store_true")
    args, rest = ap.parse_known_args()
    prescribed()
    if args.clip_range:
        clip_range(*args.clip_range)
    import eval as E
    E.main(rest)
    if args.and_without:
        E.main(rest + ["data.native_eval=false"])


if __name__ == "__main__":
    main()
