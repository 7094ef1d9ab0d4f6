"""The host decisions of the face stage (csrc/face_plan.h) without a GPU: the plan alone in a program of its own under
AddressSanitizer and UBSan, and that it stays plain host code."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_plan_alone_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/face_plan_check.cpp, built as tests/test_view_plan_cpu.py builds its program; a plain build where the
    sanitizer runtimes cannot be linked."""
    exe = str(tmp_path / "face_plan_check")
    src = os.path.join(ROOT, "tests", "cpp", "face_plan_check.cpp")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", src, "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if san.returncode != 0:
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, "the build failed:\n" + san.stderr + plain.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and " 0 failures" in run.stdout, run.stdout + run.stderr
    m = re.search(r"(\d+) steps, (\d+) checks, 0 failures", run.stdout)
    assert m and int(m.group(1)) > 16000000 and int(m.group(2)) > 33000000, run.stdout   # the program did run its cases


def test_the_plan_is_plain_host_code():
    text = open(os.path.join(ROOT, "rs-face-detection_amd", "csrc", "face_plan.h")).read()
    includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', text)
    assert includes and not [i for i in includes if "hip" in i.lower() or i in ("rfd_common.h", "kernels.h", "host_resources.h")], includes
