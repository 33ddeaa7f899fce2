"""csrc/icp_math.h under the host sanitizers, no GPU needed: tests/host_icp_math.cpp with -DICP_MATH_MAIN is a program of its own (41
iterations of transform, moments, step and keep-best on exactly sized heap buffers), built by g++ with -fsanitize=address,undefined, the
runtimes linked into the program itself, and run as a child process.  A read or write outside a buffer, or undefined arithmetic, ends it
with a report and a non-zero status."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_icp_math_program_runs_clean_under_asan_and_ubsan():
    out = os.path.join(HERE, '_build')
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, 'host_icp_math_sanitized')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined', '-static-libasan',
                           '-static-libubsan', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer', '-DICP_MATH_MAIN',
                           os.path.join(HERE, 'host_icp_math.cpp'), '-o', exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    text = r.stdout.decode()
    assert r.returncode == 0, text
    assert 'kept iteration 40' in text and 'ERROR' not in text and 'runtime error' not in text
