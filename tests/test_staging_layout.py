"""CPU: the layout object of the one-shot batch calls (qsp_slam_amd/csrc/staging_layout.hpp, no HIP in it), through
tests/staging_layout_check.cpp: a stand-alone program (sanitised), never loaded into Python."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_offsets_regions_and_total():
    with tempfile.TemporaryDirectory(prefix="qsp_staging_layout_") as tmp:
        exe = os.path.join(tmp, "check")
        san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + san
                              + ["-I" + os.path.join(ROOT, "qsp_slam_amd", "csrc"), os.path.join(ROOT, "tests", "staging_layout_check.cpp"),
                                 "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        assert r.stdout.strip() == "ok"
