"""The HIP-free job-setup code on the CPU (tests/support/heap_host_check.cpp):

* the pSync message board (csrc/psync_board.hpp) with threads as PEs: exact
  bytes from every member, one verdict everywhere, 100 rounds on one pSync
  with no stale message, words 0..15 untouched, words 16..63 zero after close
  and after an abandoned round, and the barrier counts of the setup calls
  (2 without the status phase, 3 with it, 5 for a fresh heap);
* the descriptor channel (csrc/fd_channel.cpp) on both sides of the 64 batch,
  its server's stop, a missing server, and a sender that stops half way
  (no descriptor left open);
* chunk_lens and the preflight report's exact text (csrc/heap_host.hpp).

Each case runs the program as a child process, once built plain and once
with AddressSanitizer + UBSan, which must report nothing.
"""
import subprocess

import pytest

from support import host_check_build

CASES = ["board1", "board2", "board5", "fds1", "fds64", "fds65", "fds129", "idle_server",
         "no_server", "truncated", "chunks", "report"]


@pytest.fixture(scope="module", params=["plain", "san"])
def program(request):
    return host_check_build.build("heap_host", san=request.param == "san")


@pytest.mark.parametrize("case", CASES)
def test_heap_host(program, case):
    p = subprocess.run([program, case], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout[-3000:]


def test_unknown_case_fails(program):
    assert subprocess.run([program, "nothing"], stdout=subprocess.DEVNULL,
                          stderr=subprocess.DEVNULL).returncode == 1
