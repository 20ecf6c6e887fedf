"""The owners of the library's device memory and events without a GPU: mapad_amd/csrc/lib_buffers.hpp compiled against counting stand-ins for the runtime
(tests/emu/buffers_selftest.cpp, a stand-alone program built with the address and undefined-behaviour sanitizers)."""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))


def test_owners_selftest_under_sanitizers(tmp_path):
    """growth by the rounding rule with the old block freed once; a failed allocation gives MAPAD_ERR_NOMEM, an empty buffer and no error left behind, and a later
    ensure works; release() twice; move construction, move assignment onto a full buffer, swap; an event is created once, and again after reset(); arrays of
    owners going out of scope; at the end every stand-in has got back what it gave out — in a child process of its own"""
    exe = str(tmp_path / "buffers_selftest")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unused-function",
                           "-Wno-unknown-pragmas", "-o", exe, os.path.join(_HERE, "emu", "buffers_selftest.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "buffers selftest ok" in out.stdout, out.stdout + out.stderr
