"""CPU tier of is3d_sample_decayed's host + device arithmetic (is3d2_amd/csrc/sample_decay_plan.h) and of the
SampledList transition the call makes: the stand-alone program tests/native/sample_decay_plan_check.cpp checks the
in-event index of every kept record of random sampler batches against a brute-force walk (empty events and cells, events
split over 2-5 cell windows), the 2^32 refusal, the sub-range planner and the getter codes.  It is built with
AddressSanitizer and UBSan and run as a subprocess."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "sample_decay_plan_check.cpp")


def test_in_event_indices_sub_ranges_and_the_decayed_transition(tmp_path):
    exe = str(tmp_path / "sample_decay_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, SRC])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("ok "), run.stdout + run.stderr
    assert run.stderr == "", run.stderr
