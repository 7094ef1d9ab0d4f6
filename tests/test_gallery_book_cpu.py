"""The gallery's host bookkeeping (csrc/gallery_book.h: live words, removed and labelled counts, the lazily synchronised device
words, identities, the layout of an edit slot) without a GPU: the book alone against a naive model of one bool and one int per
row, in a program of its own built with the host compiler under AddressSanitizer and UBSan."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_book_alone_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/gallery_book_check.cpp: galleries of 1 .. 4 097 rows filled exactly and one row beyond, edit chunks of 1, 1 023,
    1 024 and 1 025 rows, the slot's worst case of 4 096 ints with a guard word behind it, rows named twice or already removed,
    revived rows, refused identities, clear, the file's liveness bytes and back; then seeded random sequences; every count, bit,
    identity, slot and the device's words compared with the model after every step.  Built as tests/test_gallery_file_cpu.py
    builds its program; a plain build where the sanitizer runtimes cannot be linked."""
    exe = str(tmp_path / "gallery_book_check")
    src = os.path.join(ROOT, "tests", "cpp", "gallery_book_check.cpp")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", src, "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if san.returncode != 0:
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, "the build failed:\n" + san.stderr + plain.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and " 0 failures" in run.stdout, run.stdout + run.stderr
    m = re.search(r"(\d+) steps, (\d+) checks, 0 failures", run.stdout)
    assert m and int(m.group(1)) > 1000 and int(m.group(2)) > 100000, run.stdout   # the program did run its cases


def test_the_book_is_plain_host_code():
    """gallery_book.h includes nothing of HIP, so that a session without a GPU, and a sanitizer, can run it."""
    text = open(os.path.join(ROOT, "rs-face-detection_amd", "csrc", "gallery_book.h")).read()
    includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', text)
    assert includes and not [i for i in includes if "hip" in i.lower() or i in ("rfd_common.h", "kernels.h", "host_resources.h")], includes
