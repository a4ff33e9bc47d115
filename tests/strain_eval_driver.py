"""eval.py on the prescribed predictions of tests/strain_eval_fixture.py: started by tests/test_strain_eval_gpu.py as a fresh child process.

    python tests/strain_eval_driver.py [--clip-range LO HI] [--and-without] [eval.py's arguments ...]

tests/native_eval_driver.py's prescribed runner and clip range (the frames carry the prediction's class index; everything behind the forward
is eval.py as it stands).  --and-without runs eval.main a second time in the same process with data.lv_strain=false appended: a second JSON
line, the same run's report without the key."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import native_eval_driver as D  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clip-range", nargs=2, type=int, default=None)
    ap.add_argument("--and-without", action="store_true")
    args, rest = ap.parse_known_args()
    D.prescribed()
    if args.clip_range:
        D.clip_range(*args.clip_range)
    import eval as E
    E.main(rest)
    if args.and_without:
        E.main(rest + ["data.lv_strain=false"])


if __name__ == "__main__":
    main()
