"""CPU tier of is3d2_amd/csrc/sampled_list.h, the one owner of a sampled or decayed particle list: the stand-alone
program tests/native/sampled_list_check.cpp walks a SampledList through every transition (fresh, list-only, binned-only,
binned with the list, PTMA, decayed, new bins, a failed call) and asserts the code of every getter in each state, the
range checks and the fixed-point vn conversion.  It is built with AddressSanitizer and UBSan and run as a subprocess."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "sampled_list_check.cpp")


def test_every_getter_code_in_every_state_of_a_sampled_list(tmp_path):
    exe = str(tmp_path / "sampled_list_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, SRC])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("ok "), run.stdout + run.stderr
    assert run.stderr == "", run.stderr
