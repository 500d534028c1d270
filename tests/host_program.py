"""The stand-alone programs of tests/host/ that run the share check family's
device arithmetic on the CPU: compiled once per fixture, plainly or under
ASan + UBSan, and fed lines on stdin."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def compile_program(tmp_dir, name, flags=()):
    """tests/host/<name>.cpp compiled into tmp_dir with `flags` -> run(lines) -> its stdout lines."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_dir / name)
    cmd = [cxx, "-std=c++17", "-O1", "-g", *flags, "-I", os.path.join(ROOT, "delta-node_amd", "csrc"), "-I",
           os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", name + ".cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr

    def run(lines):
        done = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert done.returncode == 0, done.stdout + done.stderr
        return done.stdout.splitlines()

    return run


def share_lines(t, xs, rows=()):
    """The input both programs read: "<threshold> <k> <x_1> .. <x_k>", then one element's k shares per line in hex."""
    return [f"{t} {len(xs)} " + " ".join(map(str, xs))] + [" ".join(f"{y:x}" for y in ys) for ys in rows]
