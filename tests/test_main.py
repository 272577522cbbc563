"""CLI daemon end-to-end: flags, HTTP endpoints, lifecycle, stats dump
(reference analog: snap smoke test curling /metrics)."""

import json
import os
import signal
import subprocess
import sys
import time
import urllib.request

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _system_wide_perf_allowed():
    """True when this user may open system-wide perf events (root,
    CAP_PERFMON or perf_event_paranoid <= 0), probed by opening them."""
    from parca_agent_amd.native import sampler

    s = sampler().PerfSampler(freq=1, track_mmaps=False)
    try:
        s.start()
    except RuntimeError as e:
        if "permission denied" in str(e):
            return False
        raise
    finally:
        s.stop()
    return True


def _run_agent(tmp_path, *extra):
    env = dict(os.environ)
    env["PARCA_STATS_FILE"] = str(tmp_path / "stats.json")
    env["PYTHONPATH"] = REPO
    proc = subprocess.Popen(
        [sys.executable, "-m", "parca_agent_amd",
         "--http-address", "127.0.0.1:0",  # cannot scrape; use fixed port
         *extra],
        env=env, stderr=subprocess.PIPE)
    return proc


def test_version():
    out = subprocess.run(
        [sys.executable, "-m", "parca_agent_amd", "--version", "true"],
        capture_output=True, text=True, cwd=REPO)
    assert out.returncode == 0
    assert "parca-agent-amd" in out.stdout


def test_bad_flag_exit_code():
    out = subprocess.run(
        [sys.executable, "-m", "parca_agent_amd",
         "--rocm-ring-scale-factor", "99"],
        capture_output=True, text=True, cwd=REPO)
    assert out.returncode == 2


def test_daemon_lifecycle(tmp_path):
    if not _system_wide_perf_allowed():
        pytest.skip("needs system-wide perf events (root or CAP_PERFMON); "
                    "the kernel refuses them to this user")
    port = 17071
    store = tmp_path / "store"
    env = dict(os.environ)
    env["PARCA_STATS_FILE"] = str(tmp_path / "stats.json")
    env["PYTHONPATH"] = REPO
    proc = subprocess.Popen(
        [sys.executable, "-m", "parca_agent_amd",
         "--http-address", f"127.0.0.1:{port}",
         "--local-store-directory", str(store),
         "--profiling-cpu-sampling-frequency", "97",
         "--remote-store-batch-write-interval", "1s",
         "--telemetry-disable-panic-reporting", "true",
         "--analytics-opt-out", "true",
         "--rocm-enable", "false"],
        env=env, cwd=REPO, stderr=subprocess.PIPE)
    try:
        deadline = time.time() + 30
        up = False
        while time.time() < deadline:
            try:
                with urllib.request.urlopen(
                        f"http://127.0.0.1:{port}/healthz", timeout=1) as r:
                    up = r.status == 200
                    break
            except OSError:
                if proc.poll() is not None:
                    raise AssertionError(
                        proc.stderr.read().decode()[-2000:])
                time.sleep(0.2)
        assert up, "agent did not come up"

        # burn some CPU so samples accumulate
        t0 = time.time()
        while time.time() - t0 < 2.0:
            sum(range(10000))

        with urllib.request.urlopen(
                f"http://127.0.0.1:{port}/metrics", timeout=5) as r:
            metrics = r.read().decode()
        assert "parca_agent_info" in metrics
        assert "parca_agent_cpu_samples_total" in metrics

        with urllib.request.urlopen(
                f"http://127.0.0.1:{port}/debug/stats", timeout=5) as r:
            stats = json.loads(r.read())
        assert stats["cpu_samples"] > 0
    finally:
        proc.send_signal(signal.SIGTERM)
        rc = proc.wait(timeout=30)
    assert rc == 0
    # Stats dumped on shutdown.
    dumped = json.loads((tmp_path / "stats.json").read_text())
    assert dumped["cpu_samples"] > 0
    # Local store received profile batches (1s flush interval).
    files = list(store.iterdir()) if store.exists() else []
    assert any(".samples." in f.name for f in files)


def test_telemetry_supervisor_reports_panic(tmp_path):
    """--force-panic in the child must produce a ReportPanic RPC from the
    supervisor parent (reference fault injector: flags.go:413)."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from fake_parca import start_fake_parca

    fake, server, addr = start_fake_parca()
    try:
        env = dict(os.environ)
        env["PYTHONPATH"] = REPO + ":" + os.path.join(REPO, "tests")
        out = subprocess.run(
            [sys.executable, "-m", "parca_agent_amd",
             "--remote-store-address", addr,
             "--remote-store-insecure", "true",
             "--analytics-opt-out", "true",
             "--force-panic", "true"],
            env=env, cwd=REPO, capture_output=True, timeout=60)
        assert out.returncode != 0
        deadline = time.time() + 10
        while not fake.panics and time.time() < deadline:
            time.sleep(0.1)
        assert fake.panics, out.stderr.decode()[-2000:]
        stderr_text, metadata = fake.panics[0]
        assert "forced panic" in stderr_text
        assert metadata["agent_version"]
    finally:
        server.stop(grace=None)


def test_http_self_profile_endpoint(tmp_path):
    """/debug/pprof/profile self-profiles the agent with its own sampler
    (the /debug/pprof + fgprof analog, reference main.go:326-340)."""
    from parca_agent_amd.agent import Agent
    from parca_agent_amd.flags import Flags
    from parca_agent_amd.httpserver import AgentHTTPServer
    from parca_agent_amd.metrics import build_registry
    from parca_agent_amd.pprof import decode_profile

    flags = Flags()
    flags.rocm.enable = False
    agent = Agent(flags, enable_cpu=True, enable_gpu=False)
    registry = build_registry(agent)
    server = AgentHTTPServer("127.0.0.1:0", agent, registry)
    try:
        # Exercise the self-profiler directly (short window); busy-spin a
        # thread so there is something to sample.
        import threading

        stop = threading.Event()

        def burn():
            while not stop.is_set():
                sum(range(5000))

        t = threading.Thread(target=burn, daemon=True)
        t.start()
        try:
            data = server.self_profile(2)
        finally:
            stop.set()
        if data:  # perf may be restricted in exotic environments
            prof = decode_profile(data)
            assert prof.sample_types[0].type == "samples"
    finally:
        server.stop() if server._thread else server._httpd.server_close()


def test_daemon_gpu_ring_integration(tmp_path):
    """Daemon end-to-end with a synthetic GPU event ring (no GPU): the
    gpu service must pick up the ring and the local store must receive a
    gpu_kernel_time pprof."""
    from parca_agent_amd.gpu import events as ev
    from parca_agent_amd.native import gpu as native_gpu
    from parca_agent_amd.pprof import decode_profile

    g = native_gpu()
    shm = tmp_path / "shm"
    shm.mkdir()
    store = tmp_path / "store"
    pid = os.getpid()  # alive, so the daemon won't reap the ring
    prod = g.TestRingProducer(str(shm / f"parca_gpu_{pid}.ring"), 1 << 20)
    prod.write(g.EV_KERNEL_SYMBOL, ev.encode_kernel_symbol(
        ev.KernelSymbol(kernel_id=1, code_object_id=1, kernel_object=0,
                        name="integration_kernel")))
    prod.write(g.EV_KERNEL_DISPATCH, ev.encode_kernel_dispatch(
        ev.KernelDispatch(
            correlation_id=1, dispatch_id=1, kernel_id=1,
            start_ns=1000, end_ns=51000, tid=pid, gpu_index=0, pid=pid,
            grid=(1, 1, 1), workgroup=(64, 1, 1),
            private_segment_size=0, group_segment_size=0)))

    env = dict(os.environ)
    env["PYTHONPATH"] = REPO
    proc = subprocess.Popen(
        [sys.executable, "-m", "parca_agent_amd",
         "--http-address", "127.0.0.1:17072",
         "--local-store-directory", str(store),
         "--remote-store-batch-write-interval", "1s",
         "--rocm-shm-dir", str(shm),
         "--telemetry-disable-panic-reporting", "true",
         "--analytics-opt-out", "true"],
        env=env, cwd=REPO, stderr=subprocess.PIPE)
    try:
        deadline = time.time() + 45
        found = None
        while time.time() < deadline and not found:
            if proc.poll() is not None:
                raise AssertionError(proc.stderr.read().decode()[-2000:])
            if store.exists():
                for f in store.iterdir():
                    if ".gpu_kernel_time." in f.name:
                        found = f
                        break
            time.sleep(0.5)
        assert found, "no gpu_kernel_time profile produced"
        prof = decode_profile(found.read_bytes())
        names = set()
        for s in prof.samples:
            names.update(prof.stack_names(s))
        assert "integration_kernel" in names
        [sample] = [s for s in prof.samples
                    if "integration_kernel" in prof.stack_names(s)]
        assert sample["values"] == [50000]
    finally:
        proc.send_signal(signal.SIGTERM)
        proc.wait(timeout=30)


def test_preflight_tool():
    """tools/preflight.py must run FAIL-free wherever the agent can do
    all of its work. The one capability a checkout cannot bring along is
    the privilege for system-wide perf events: where the kernel really
    refuses them, preflight must report exactly that FAIL and no other."""
    import subprocess
    import sys

    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "tools", "preflight.py")],
        capture_output=True, text=True, timeout=120)
    fails = [ln for ln in out.stdout.splitlines() if ln.startswith("[FAIL]")]
    if _system_wide_perf_allowed():
        assert out.returncode == 0, out.stdout + out.stderr
        assert '"fail": 0' in out.stdout
        assert fails == []
    else:
        assert out.returncode == 1, out.stdout + out.stderr
        assert '"fail": 1' in out.stdout
        assert len(fails) == 1 and \
            "perf_event system-wide sampling" in fails[0], out.stdout


def test_report_tool(tmp_path):
    """tools/report.py renders top-N tables from local-store pprof."""
    import shutil
    import subprocess
    import sys

    shutil.copy(os.path.join(REPO, "profiles", "gemm_loop.samples.pb.gz"),
                tmp_path / "1.samples.pb.gz")
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "tools", "report.py"),
         str(tmp_path), "-n", "3", "--cum"],
        capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert "top 3 (cum):" in out.stdout
    assert "%" in out.stdout


def test_fgprof_wallclock_endpoint():
    """/debug/pprof/fgprof returns a wallclock profile of agent threads
    including blocked ones (reference serves fgprof, main.go:332)."""
    import threading
    import urllib.request

    from prometheus_client import CollectorRegistry

    from parca_agent_amd.httpserver import AgentHTTPServer
    from parca_agent_amd.pprof.profile import decode_profile

    ev = threading.Event()
    t = threading.Thread(target=lambda: wait_for_test_marker(ev),
                         name="blocked-worker", daemon=True)
    t.start()

    class A:
        def stats(self):
            return None

    srv = AgentHTTPServer("127.0.0.1:0", A(), CollectorRegistry())
    srv.start()
    try:
        data = urllib.request.urlopen(
            f"http://127.0.0.1:{srv.port}/debug/pprof/fgprof?seconds=1",
            timeout=30).read()
    finally:
        ev.set()
        srv.stop()
    p = decode_profile(data)
    names = set()
    threads = set()
    for s in p.samples:
        names.update(p.stack_names(s))
        threads.add(s["labels"].get("thread_name", ""))
    # The deliberately blocked thread must appear with its wait frame —
    # that is what wallclock gives over on-CPU.
    assert "wait_for_test_marker" in names, sorted(names)[:10]
    assert "blocked-worker" in threads


def wait_for_test_marker(ev):
    ev.wait(30)
