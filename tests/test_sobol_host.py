"""The host arithmetic of scfgp_sobol in scfgp_amd/csrc/api_host.h on its own: tests/host/sobol_host_check.cpp (a program with its own
main; no library, no GPU) built with the host compiler, once plain and once with -fsanitize=address,undefined, and both binaries run
directly (tests/test_api_host.py's pattern)."""
import os
import subprocess

import pytest

from tests.test_api_host import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'host', 'sobol_host_check.cpp')


@pytest.mark.parametrize('flags', [(), ('-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-g')], ids=['plain', 'asan_ubsan'])
def test_sobol_host_check(tmp_path, flags):
    exe = str(tmp_path / 'sobol_host_check')
    cmd = [_compiler(), '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror'] + list(flags) + [SRC, '-o', exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == 'ok', r.stdout[-4000:]
    assert 'runtime error' not in r.stdout and 'AddressSanitizer' not in r.stdout
