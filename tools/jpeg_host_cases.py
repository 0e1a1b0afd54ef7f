"""Writes Pillow-encoded baseline JPEG files (tests/jpeg_cases.py's generator) into a temporary directory and runs
tools/micro/jpeg_host on them: the host parser and the entropy decode's per-thread arithmetic under AddressSanitizer, on the valid
files and on truncated and byte-flipped copies the program makes itself (build it first: make -C tools/micro jpeg_host).  No GPU.
usage: python tools/jpeg_host_cases.py"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_cases as jc  # noqa: E402


def main():
    exe = os.path.join(ROOT, "tools", "micro", "jpeg_host")
    if not os.path.exists(exe):
        sys.exit("build it first: make -C tools/micro jpeg_host")
    with tempfile.TemporaryDirectory() as d:
        files = []
        for (w, h) in [(17, 13), (40, 52), (33, 47)]:
            for s in jc.SAMPLINGS:
                for q in (30, 100):
                    for m in jc.MODES + ["restart1"]:
                        files.append((f"{w}x{h}_{s.replace(':', '')}_q{q}_{m}.jpg", jc.case(w, h, s, q, "noise", m)))
        files.append(("stuffed.jpg", jc.stuffed_case()[0]))
        files.append(("large_noise.jpg", jc.case(256, 192, "4:2:0", 95, "noise")))
        files.append(("large_smooth.jpg", jc.case(256, 192, "4:2:0", 30, "smooth")))
        paths = []
        for name, data in files:
            paths.append(os.path.join(d, name))
            with open(paths[-1], "wb") as f:
                f.write(data)
        sys.exit(subprocess.run([exe] + paths).returncode)


if __name__ == "__main__":
    main()
