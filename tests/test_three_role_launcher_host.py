"""Host: the failure path of tests/secure_common.py's run_roles, which starts and supervises the three roles of every
three-role GPU test.  Three small Python children that import nothing heavy stand in for the roles; each test keeps failures in
a list of its own, never in the session's."""
import os
import sys
import time

import pytest

from tests.secure_common import run_roles


def child(code):
    return [sys.executable, "-c", code]


def test_a_failed_role_ends_its_peers_and_is_named(tmp_path):
    """Rank 1 exits with 3 after 0.2 s while its peers would sleep for a minute: they are terminated, not waited out (nor left
    to their 30 s limit); the report names rank 1 and its status, and the failure is kept."""
    failures = []
    cmds = [child("import time; time.sleep(60)"), child("import sys, time; time.sleep(0.2); sys.exit(3)"),
            child("import time; time.sleep(60)")]
    t0 = time.monotonic()
    with pytest.raises(AssertionError, match="rank 1 exited with 3") as err:
        run_roles(cmds, str(tmp_path / "roles"), limit=30, failures=failures, what="one fails")
    assert time.monotonic() - t0 < 15
    assert failures == ["one fails: rank 1 exited with 3"]
    assert "(1, 3," in str(err.value)
    assert all(os.path.exists(tmp_path / f"roles.log{r}") for r in range(3))


def test_a_role_past_its_limit_is_reported_with_124(tmp_path):
    failures = []
    cmds = [child("print('done')"), child("print('done')"), child("import time; time.sleep(60)")]
    t0 = time.monotonic()
    with pytest.raises(AssertionError, match="rank 2 exited with 124"):
        run_roles(cmds, str(tmp_path / "roles"), limit=2, failures=failures, what="too long")
    assert 2 <= time.monotonic() - t0 < 15
    assert failures == ["too long: rank 2 exited with 124"]


def test_after_a_failure_nothing_is_started_and_success_returns_every_status(tmp_path):
    marker = tmp_path / "started"
    touch = child(f"open({str(marker)!r}, 'w').close()")
    with pytest.raises(AssertionError, match="an earlier three-role run failed .earlier: rank 0 exited with 1."):
        run_roles([touch] * 3, str(tmp_path / "refused"), failures=["earlier: rank 0 exited with 1"])
    assert not marker.exists() and not os.path.exists(tmp_path / "refused.log0")
    failures = []
    hello = child("import os; print('rank', os.environ['RANK'], 'of', os.environ['WORLD_SIZE'], os.environ['MASTER_PORT'])")
    results = run_roles([hello] * 3, str(tmp_path / "roles"), limit=30, failures=failures)
    assert [(r, rc) for r, rc, _ in results] == [(0, 0), (1, 0), (2, 0)] and failures == []
    ports = set()
    for r, _, text in results:
        assert text.startswith(f"rank {r} of 3 ")
        assert open(tmp_path / f"roles.log{r}").read() == text
        ports.add(text.split()[-1])
    assert len(ports) == 1
