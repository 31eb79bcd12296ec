"""The co-residency guards (csrc/device_share.h) checked without a GPU: the inter-process device lease, the
device-users markers with the automatic switch to shared-device mode, the mode's own state, and the in-process gate.

The header is host code over POSIX files and std::mutex: tests/device_share_check.cpp drives it, compiled here with g++,
over directories of tmp_path.  This file plays "the other process" with fcntl.flock and os.utime.  What is pinned here
is the on-disk protocol that builds of the library share: file names, what a planted name does, modes,
the 0.3 s / 2 s marker rules, the scan schedule, the lease's bounded wait -- and the gate's admission rule, against a
pretended device whose launches check the rule themselves.  tests/test_gpu_shared.py runs the same guards around real
kernels."""
import fcntl
import os
import stat
import subprocess
import threading
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stanford-ctc_amd", "csrc")
KEY = "0000_c1_00_0"
NOT_OBTAINED = ("sctc: device lease not obtained within 0 s (another process holds the GPU's persistent-launch lock): "
                "this step runs on the per-step recurrent kernels\n")
SWITCHED_ON = ("sctc: 3 processes run persistent kernels on this GPU: shared-device mode on "
               "(their launches take turns under /dev/shm/sctc_gpu_*.lock)\n")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("device_share") / "device_share_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-pthread", "-I", CSRC,
                           os.path.join(ROOT, "tests", "device_share_check.cpp"), "-o", exe])
    return exe


class Dirs:
    def __init__(self, tmp_path, make=True):
        self.a, self.b, self.m = (str(tmp_path / n) for n in ("lease1", "lease2", "markers"))
        os.mkdir(self.m)
        self.fds = []
        if make:
            self.make_lease_dirs()

    def make_lease_dirs(self):
        os.mkdir(self.a)
        os.mkdir(self.b)

    def lock(self, which, key=KEY):
        return os.path.join(which, "sctc_gpu_%s.lock" % key)

    def marker(self, pid, key=KEY):
        return os.path.join(self.m, "sctc_gpu_%s.user.%d" % (key, pid))

    def plant_marker(self, pid, age, locked, key=KEY):
        """another process's marker, its mtime `age` seconds back, locked until the test is over"""
        fd = os.open(self.marker(pid, key), os.O_CREAT | os.O_RDWR, 0o666)
        if locked:
            fcntl.flock(fd, fcntl.LOCK_EX)
        t = time.time() - age
        os.utime(self.marker(pid, key), (t, t))
        self.fds.append(fd)


@pytest.fixture
def d(tmp_path):
    dirs = Dirs(tmp_path)
    yield dirs
    for fd in dirs.fds:
        os.close(fd)


class Session:
    """`device_share_check session` answering one line per command; a process that hangs is killed after 10 s"""
    def __init__(self, check, d, wait_s=30, shared_device=None, umask=-1):
        env = dict(os.environ)
        env.pop("SCTC_SHARED_DEVICE", None)
        if shared_device is not None:
            env["SCTC_SHARED_DEVICE"] = shared_device
        self.proc = subprocess.Popen([check, "session", d.a, d.b, d.m, str(wait_s)], stdin=subprocess.PIPE,
                                     stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=env,
                                     umask=umask)
        self.pid = self.proc.pid
        self.timer = threading.Timer(10, self.proc.kill)
        self.timer.start()

    def ask(self, command):
        self.proc.stdin.write(command + "\n")
        self.proc.stdin.flush()
        line = self.proc.stdout.readline()
        assert line.endswith("\n"), "no answer to %r" % command
        return line[:-1]

    def lease(self, key=KEY):
        locked, waited, umask = (x.split("=")[1] for x in self.ask("lease " + key).split())
        return int(locked), float(waited), int(umask, 8)

    def close(self):
        """-> what the process wrote to stderr"""
        _, err = self.proc.communicate()
        self.timer.cancel()
        assert self.proc.returncode == 0
        return err

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self.proc.returncode is None:
            self.proc.kill()
            self.proc.communicate()
        self.timer.cancel()


def mode_of(path):
    return stat.S_IMODE(os.stat(path).st_mode)


# ---------------------------------------------------------------- names

def test_names(check, d):
    with Session(check, d) as s:
        assert s.ask("key 0000:c1:00.0") == KEY
        assert s.ask("key a/b.c:d") == "a_b_c_d"
        assert s.ask("key EMPTY") == "unknown"
        assert s.ask("key NULL") == "unknown"
        assert s.ask("paths " + KEY) == "%s/sctc_gpu_%s.lock %s/sctc_gpu_%s.lock %s/sctc_gpu_%s.user.%d" % (
            d.a, KEY, d.b, KEY, d.m, KEY, s.pid)
        assert s.close() == ""
    out = subprocess.run([check, "defaults"], stdout=subprocess.PIPE, check=True, universal_newlines=True, timeout=10).stdout
    assert out == "/dev/shm/sctc_gpu_KEY.lock /tmp/sctc_gpu_KEY.lock /dev/shm/sctc_gpu_KEY.user.PID 30 0.3 2\n"


# ---------------------------------------------------------------- the lease

def test_lease_excludes_processes_and_threads(check, tmp_path):
    counter = str(tmp_path / "counter")
    with open(counter, "w") as f:
        f.write("0\n")
    procs = [subprocess.Popen([check, "hammer", str(tmp_path), counter], stdout=subprocess.PIPE, universal_newlines=True)
             for _ in range(2)]
    for p in procs:
        assert p.communicate(timeout=20)[0] == "failed=0\n" and p.returncode == 0
    assert open(counter).read() == "200\n"


def test_lease_wait_is_bounded(check, d):
    other = os.open(d.lock(d.a), os.O_CREAT | os.O_RDWR, 0o666)
    d.fds.append(other)
    fcntl.flock(other, fcntl.LOCK_EX)
    with Session(check, d, wait_s=0.3) as s:
        locked, waited, _ = s.lease()
        assert locked == 0 and waited >= 0.3
        fcntl.flock(other, fcntl.LOCK_UN)
        assert s.lease()[0] == 1
        assert s.close() == NOT_OBTAINED
    assert not os.path.exists(d.lock(d.b))      # a held lock is waited for, not walked around


@pytest.mark.parametrize("planted", ["symlink", "directory"])
def test_planted_name_is_not_followed(check, tmp_path, d, planted):
    victim = str(tmp_path / "victim")
    with open(victim, "w") as f:
        f.write("victim")
    os.chmod(victim, 0o600)
    if planted == "symlink":
        os.symlink(victim, d.lock(d.a))
    else:
        os.mkdir(d.lock(d.a))
    with Session(check, d) as s:
        assert s.lease()[0] == 1
        assert s.close() == ""
    assert os.path.isfile(d.lock(d.b)) and not os.path.islink(d.lock(d.b))
    assert open(victim).read() == "victim" and mode_of(victim) == 0o600
    assert os.path.islink(d.lock(d.a)) if planted == "symlink" else os.path.isdir(d.lock(d.a))


def test_no_usable_directory_is_remembered(check, tmp_path):
    d = Dirs(tmp_path, make=False)
    with Session(check, d) as s:
        assert s.lease()[0] == 0
        d.make_lease_dirs()
        assert s.lease()[0] == 0                # no second open: the first answer holds for the process
        assert os.listdir(d.a) == [] and os.listdir(d.b) == []
        assert s.lease("another_device")[0] == 1
        assert s.close() == ""


def test_own_narrow_file_is_widened_and_umask_kept(check, d):
    fd = os.open(d.lock(d.a), os.O_CREAT | os.O_RDWR)
    os.fchmod(fd, 0o600)
    os.close(fd)
    with Session(check, d, umask=0o027) as s:
        assert s.lease()[::2] == (1, 0o027)
        assert mode_of(d.lock(d.a)) == 0o666
        assert s.lease("fresh")[::2] == (1, 0o027)      # created under umask 027, widened on the descriptor
        assert mode_of(d.lock(d.a, "fresh")) == 0o666
        assert s.ask("count " + KEY) == "1"
        assert mode_of(d.marker(s.pid)) == 0o666
        assert s.lease()[2] == 0o027
        assert s.close() == ""


# ---------------------------------------------------------------- the markers

# mtimes: 5 s in the future is "fresh" however loaded the machine is; 1 s back is idle (> 0.3 s); 3 s back is stale (> 2 s)
@pytest.mark.parametrize("locked,age,count,stays", [(True, -5, 2, True), (True, 1, 1, True), (False, 3, 1, False),
                                                    (False, -5, 1, True)])
def test_foreign_marker(check, d, locked, age, count, stays):
    d.plant_marker(1000001, age, locked)
    with Session(check, d) as s:
        assert s.ask("count " + KEY) == str(count)
        assert os.path.exists(d.marker(1000001)) == stays
        assert s.close() == ""


def test_marker_of_another_device_is_ignored(check, d):
    d.plant_marker(1000001, -5, True, key=KEY + "x")
    d.plant_marker(1000002, -5, True, key="0000_c2_00_0")
    d.plant_marker(1000003, 3, False, key="0000_c2_00_0")
    with Session(check, d) as s:
        assert s.ask("count " + KEY) == "1"
        assert s.close() == ""
    assert os.path.exists(d.marker(1000003, key="0000_c2_00_0"))


def test_own_marker(check, d):
    with Session(check, d) as s:
        own = d.marker(s.pid)
        assert s.ask("due %s 1" % KEY) == "1" and not os.path.exists(own)      # made by the first scan, not before
        assert s.ask("count " + KEY) == "1"
        fd = os.open(own, os.O_RDWR)
        with pytest.raises(BlockingIOError):
            fcntl.flock(fd, fcntl.LOCK_SH | fcntl.LOCK_NB)
        long_ago = time.time() - 100
        os.utime(own, (long_ago, long_ago))
        assert s.ask("due %s 1" % KEY) == "1"
        assert os.stat(own).st_mtime > long_ago + 50
        assert s.ask("count " + KEY) == "1"     # the marker it holds, not a second one
        assert s.close() == ""
        fcntl.flock(fd, fcntl.LOCK_SH | fcntl.LOCK_NB)     # the process is gone: so is its lock
    assert os.listdir(d.m) == [os.path.basename(own)]


def test_scan_schedule(check, d):
    with Session(check, d) as s:
        want = "".join("1" if (k in (1, 2, 4, 8, 16, 32) or k % 32 == 0) else "0" for k in range(1, 201))
        assert s.ask("due %s 200" % KEY) == want
        assert s.ask("due other 3") == "110"    # counted per device


# ---------------------------------------------------------------- the mode

@pytest.mark.parametrize("first", ["get", "set"])
@pytest.mark.parametrize("env", [None, "0", "1"])
def test_mode_state_and_automatic_switch(check, d, env, first):
    d.plant_marker(1000001, -5, True)
    d.plant_marker(1000002, -5, True)
    named = int(env is not None)
    with Session(check, d, shared_device=env) as s:
        if first == "get":
            start = int(env == "1")
            assert s.ask("mode") == "mode=%d env_named=%d" % (start, named)
        else:
            start = 0
            assert s.ask("set 0") == "mode=0 env_named=%d" % named
        # the switch is the library's own only when the environment did not name the mode
        after = 1 if env is None else start
        assert s.ask("launch " + KEY) == str(after)
        assert s.ask("mode") == "mode=%d env_named=%d" % (after, named)
        assert os.path.exists(d.marker(s.pid)) == (env is None)       # no scan, no marker
        assert s.ask("set 1") == "mode=1 env_named=%d" % named
        assert s.ask("set 0") == "mode=0 env_named=%d" % named
        assert s.ask("set 7") == "mode=1 env_named=%d" % named
        assert s.close() == (SWITCHED_ON if env is None else "")


def test_alone_on_the_device_the_mode_stays_off(check, d):
    d.plant_marker(1000001, 1, True)        # somebody who exists but launches nothing
    with Session(check, d) as s:
        assert [s.ask("launch " + KEY) for _ in range(40)] == ["0"] * 40
        assert s.close() == ""


# ---------------------------------------------------------------- the gate

def test_gate(check):
    out = subprocess.run([check, "gate"], stdout=subprocess.PIPE, check=True, universal_newlines=True, timeout=20).stdout
    lines = dict(line.split(": ") for line in out.splitlines())
    # B does not fit next to A: it waits for A's event, once, and then takes that event over
    assert lines["two_whole_device_grids"] == "rc=0 waits=1 event0 launches=2 events=1 inflight=1 violations=0"
    assert lines["two_small_grids"] == "rc=0 waits=0 launches=2 events=2 inflight=2 violations=0"
    assert lines["one_stream"] == "rc=0 waits=0 launches=3 events=3 inflight=3 violations=0"
    assert lines["failed_launch"] == "rc=5 waits=0 launches=0 events=0 inflight=0 violations=0"
    assert lines["event_reuse"] == "rc=0 events=10 max_inflight=10"
    t = dict((k, int(v)) for k, v in (x.split("=") for x in lines["threads"].split()))
    assert t["failed"] == 0 and t["launches"] == 800 and t["violations"] == 0
    assert 1 <= t["events"] <= t["max_inflight"]
