"""The host side of the R1CS -> QAP build (csrc/qap_csc.h: validation and the CSR -> column-wise counting sort) under the host sanitizers: a stand-alone
program (tests/c/qap_csc_check.cpp, its own main) is compiled with -fsanitize=address,undefined and run.  No GPU, nothing loaded into python."""
import os, shutil, subprocess
from zkt_testlib import ROOT


def test_qap_csc_header_under_address_and_undefined_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    static_rt = ["-static-libasan", "-static-libubsan"] if cxx.endswith("g++") and "clang" not in cxx else []      # the runtimes inside the program: it runs as it is, whatever the loader preloads
    exe = tmp_path / "qap_csc_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static_rt,
                           "-I", os.path.join(ROOT, "zk-toolkit_amd", "csrc"), os.path.join(ROOT, "tests", "c", "qap_csc_check.cpp"), "-o", str(exe)], timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "qap_csc ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
