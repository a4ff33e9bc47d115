"""Is the gfx950 device code of every csrc/*.hip the same as at a git revision?  `python tools/isa_equal.py [REV]` (default HEAD).

Unpacks REV's gdkvm_amd/csrc and include into a temporary directory, compiles every .hip of that tree and of the working tree to device
assembly with the build's own flags, drops the per-translation-unit `__hip_cuid_<hash>` lines and compares the rest.  One line per file,
`identical` or `differs: N lines`; exit status 1 if any file differs.  Needs no GPU.

`--kernels`: for a file that differs, say which of REV's kernels no longer exist instruction for instruction.  A kernel's text is taken
from its label to `.end_amdhsa_kernel` with its own symbol, the function index in `.LBB<n>_` / `.Lfunc_end<n>` labels and runs of
blanks normalised, and looked up among the working tree's kernels of that file: a template that gained a parameter (new mangled
names) or a file that gained kernels (renumbered labels) then still reports every old kernel as `kept`."""
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdkvm_amd import build  # noqa: E402


def device_asm(root, name, out):
    """Device assembly lines of <root>/gdkvm_amd/csrc/<name> under the build's flags.  The quoted includes of a .hip find the headers beside
    it first, and <root>/include goes in front of the build's own -I, so each tree is compiled against its own headers."""
    cmd = [build.HIPCC, "-I" + os.path.join(root, "include")] + build.FLAGS + build.EXTRA_FLAGS.get(name, []) + ["--cuda-device-only", "-S"]
    subprocess.check_call(cmd + [os.path.join(root, "gdkvm_amd", "csrc", name), "-o", out])
    with open(out) as f:
        return [line for line in f if "__hip_cuid_" not in line]


def kernel_bodies(lines):
    """{symbol: normalised text} of the kernels in a device assembly listing."""
    out, name, body = {}, None, []
    for line in lines:
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
        elif name is not None:
            body.append(re.sub(r"\s+", " ", re.sub(r"L?BB\d+_|Lfunc_end\d+", "L", line.replace(name, "K"))))
            if ".end_amdhsa_kernel" in line:
                out[name] = "\n".join(body)
                name = None
    return out


def main():
    by_kernel = "--kernels" in sys.argv
    sys.argv = [a for a in sys.argv if a != "--kernels"]
    rev = sys.argv[1] if len(sys.argv) > 1 else "HEAD"
    print(subprocess.check_output([build.HIPCC, "--version"], text=True).splitlines()[0])
    with tempfile.TemporaryDirectory() as tmp:
        old = os.path.join(tmp, "old")
        os.makedirs(old)
        tar = subprocess.Popen(["git", "-C", build.ROOT, "archive", rev, "gdkvm_amd/csrc", "include"], stdout=subprocess.PIPE)
        subprocess.check_call(["tar", "-x", "-C", old], stdin=tar.stdout)
        if tar.wait() != 0:
            raise SystemExit(f"git archive {rev} failed")
        names = [os.path.basename(s) for s in build.sources()]
        gone = sorted(set(n for n in os.listdir(os.path.join(old, "gdkvm_amd", "csrc")) if n.endswith(".hip")) ^ set(names))
        with ThreadPoolExecutor(max_workers=16) as pool:         # each worker waits on one hipcc: at most 16 compilers at a time
            jobs = {n: (pool.submit(device_asm, old, n, os.path.join(tmp, "old_" + n + ".s")),
                        pool.submit(device_asm, build.ROOT, n, os.path.join(tmp, "new_" + n + ".s"))) for n in names if n not in gone}
            bad = len(gone)
            for n in gone:
                print(f"{n}: in one tree only")
            for n, (a, b) in jobs.items():
                a, b = a.result(), b.result()
                d = sum(1 for line in difflib.unified_diff(a, b, n=0) if line[0] in "+-" and line[:3] not in ("+++", "---"))
                print(f"{n}: " + (f"differs: {d} lines" if d else "identical"), flush=True)
                bad += d != 0
                if d and by_kernel:
                    old_k, new_k = kernel_bodies(a), kernel_bodies(b)
                    have = set(new_k.values())
                    for sym, text in old_k.items():
                        print(f"    {'kept   ' if text in have else 'CHANGED'} {sym}")
                    print(f"    {len(new_k) - sum(1 for t in new_k.values() if t in set(old_k.values()))} kernel(s) only in the working tree")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
