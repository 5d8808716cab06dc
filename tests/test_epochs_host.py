"""csrc/epochs.h -- which geometry epoch's lists a plan's slots hold and which epoch's background its shallow buffers hold --
is plain C++: tests/host/epochs_main.cpp exercises it as a stand-alone program built with the host sanitizers (address,
undefined behaviour).  No GPU, no library, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "2d-to-3d-style-transfer_amd", "csrc")


def _compiler():
    """the compiler the library itself is built with (build.py), on plain C++: clang links the sanitizer runtimes into the
    program, so it runs whatever else the environment loads into a process"""
    return [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "c++"]


def test_epoch_slots_and_clean_record_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "epochs_main")
    cmd = _compiler() + ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "host", "epochs_main.cpp"), "-o", exe]
    c = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "epochs ok" in r.stdout, f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
