// Drives csrc/device_share.h without a GPU (tests/test_device_share_cpu.py compiles this with g++ -pthread).
//   device_share_check session LEASE_DIR1 LEASE_DIR2 MARKER_DIR LEASE_WAIT_S
//       one DeviceShare over those directories; commands on stdin, one answer line each on stdout:
//         key ID            share_key(ID); ID "NULL" is the null pointer, "EMPTY" the empty string
//         paths KEY         the lock path in each lease directory and the own marker's path
//         lease KEY         a LeaseGuard: "locked=0|1 waited=SECONDS umask=OCTAL" (umask read after the guard is gone)
//         count KEY         DeviceUsers::count
//         due KEY N         N calls of DeviceUsers::due: a string of N characters 0 / 1
//         mode              SharedMode::get and env_named
//         set V             SharedMode::set(V), then as `mode`
//         launch KEY        DeviceShare::shared_for_launch
//   device_share_check hammer DIR COUNTER_FILE
//       two threads x 50 unlocked read-modify-write increments of COUNTER_FILE, each under a LeaseGuard
//   device_share_check gate
//       PersistentGate over fake events on a device of 256 CUs: one line per case
//   device_share_check defaults
//       the file names and time constants of the library's own DeviceShare
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <deque>
#include <random>
#include <thread>

#include "device_share.h"

using namespace sctc;

static int session(char** argv)
{
    ShareConfig cfg;
    cfg.lease_dirs = {argv[0], argv[1]};
    cfg.marker_dir = argv[2];
    cfg.lease_wait_s = atof(argv[3]);
    DeviceShare share(cfg);
    char cmd[32], arg[256];
    int n;
    auto mode = [&]() { printf("mode=%d env_named=%d\n", share.mode.get(), (int)share.mode.env_named()); };
    while (scanf("%31s", cmd) == 1) {
        if (!strcmp(cmd, "mode")) {
            mode();
        } else if (!strcmp(cmd, "set") && scanf("%d", &n) == 1) {
            share.mode.set(n);
            mode();
        } else if (scanf("%255s", arg) != 1) {
            return 2;
        } else if (!strcmp(cmd, "key")) {
            printf("%s\n", share_key(!strcmp(arg, "NULL") ? nullptr : !strcmp(arg, "EMPTY") ? "" : arg).c_str());
        } else if (!strcmp(cmd, "paths")) {
            printf("%s %s %s/%s\n", cfg.lock_path(cfg.lease_dirs[0], arg).c_str(), cfg.lock_path(cfg.lease_dirs[1], arg).c_str(),
                   cfg.marker_dir.c_str(), share.users.own_marker(arg).c_str());
        } else if (!strcmp(cmd, "lease")) {
            const double t0 = monotonic_s();
            bool locked;
            {
                LeaseGuard guard(share.lease, arg);
                locked = guard.locked;
            }
            const double waited = monotonic_s() - t0;
            const mode_t um = umask(0);
            umask(um);
            printf("locked=%d waited=%.3f umask=%03o\n", (int)locked, waited, (unsigned)um);
        } else if (!strcmp(cmd, "count")) {
            printf("%d\n", share.users.count(arg));
        } else if (!strcmp(cmd, "due") && scanf("%d", &n) == 1) {
            for (int i = 0; i < n; ++i) putchar(share.users.due(arg) ? '1' : '0');
            putchar('\n');
        } else if (!strcmp(cmd, "launch")) {
            printf("%d\n", (int)share.shared_for_launch(arg));
        } else {
            return 2;
        }
        fflush(stdout);
    }
    return 0;
}

static int hammer(const char* dir, const char* counter)
{
    ShareConfig cfg;
    cfg.lease_dirs = {dir};
    cfg.marker_dir = dir;
    DeviceShare share(cfg);
    std::atomic<int> failed{0};
    auto work = [&]() {
        for (int i = 0; i < 50; ++i) {
            LeaseGuard guard(share.lease, "0000_c1_00_0");
            long v = -1;
            FILE* f = guard.locked ? fopen(counter, "r") : nullptr;
            if (!f || fscanf(f, "%ld", &v) != 1) { ++failed; return; }
            fclose(f);
            usleep(200);    // long enough for a second writer to get in, were it let in
            f = fopen(counter, "w");
            if (!f) { ++failed; return; }
            fprintf(f, "%ld\n", v + 1);
            fclose(f);
        }
    };
    std::thread a(work), b(work);
    a.join();
    b.join();
    printf("failed=%d\n", failed.load());
    return failed.load() ? 1 : 0;
}

// Events of a pretended device.  A launch is complete when its owner says so (finish) or, in the single-threaded cases,
// when somebody waits for it.  Everything but Launch::done is touched under the gate's lock only.
struct FakeEvents {
    struct Launch { int stream, cus; std::atomic<bool> done{false}; Launch(int s, int c) : stream(s), cus(c) {} };
    typedef int Event;
    typedef int Stream;
    std::deque<Launch> launches;            // references stay valid while it grows
    std::vector<Launch*> bound;             // event -> the launch it was last recorded behind
    std::vector<Event> waited;
    int violations = 0;
    bool wait_completes = true;             // false: wait() spins until the owning thread finishes the launch

    bool done(Event e) { return bound[e]->done.load(); }
    int wait(Event e)
    {
        waited.push_back(e);
        if (wait_completes) bound[e]->done.store(true);
        while (!bound[e]->done.load()) std::this_thread::yield();
        return 0;
    }
    int create(Event* e)
    {
        bound.push_back(nullptr);
        *e = (int)bound.size() - 1;
        return 0;
    }
    int record(Event e, Stream s)
    {
        for (auto it = launches.rbegin(); it != launches.rend(); ++it)
            if (it->stream == s) { bound[e] = &*it; return 0; }
        return 7;
    }
    // what a launch callback does: the gate's promise, checked against the launches themselves
    Launch* launch(int stream, int cus, int device_cus)
    {
        int other = 0;
        for (Launch& l : launches)
            if (!l.done.load() && l.stream != stream) other += l.cus;
        if (other != 0 && other + cus > device_cus) ++violations;
        launches.emplace_back(stream, cus);
        return &launches.back();
    }
};
typedef PersistentGate<FakeEvents> FakeGate;

static int admit(FakeGate& g, int stream, int cus)
{
    return g.admit_and_launch(0, stream, cus, 256, [&]() { g.events.launch(stream, cus, 256); return 0; });
}

static void gate_report(const char* name, FakeGate& g, int rc)
{
    printf("%s: rc=%d waits=%zu", name, rc, g.events.waited.size());
    for (int e : g.events.waited) printf(" event%d", e);
    printf(" launches=%zu events=%zu inflight=%zu violations=%d\n", g.events.launches.size(), g.events.bound.size(),
           g.inflight[0].size(), g.events.violations);
}

static int gate()
{
    {
        FakeGate g;
        int rc = admit(g, 1, 228);
        if (!rc) rc = admit(g, 2, 228);
        gate_report("two_whole_device_grids", g, rc);
    }
    {
        FakeGate g;
        int rc = admit(g, 1, 100);
        if (!rc) rc = admit(g, 2, 100);
        gate_report("two_small_grids", g, rc);
    }
    {
        FakeGate g;
        int rc = 0;
        for (int i = 0; i < 3 && !rc; ++i) rc = admit(g, 1, 228);
        gate_report("one_stream", g, rc);
    }
    {
        FakeGate g;
        const int rc = g.admit_and_launch(0, 1, 228, 256, []() { return 5; });
        gate_report("failed_launch", g, rc);
    }
    {
        // ten launches that stay in flight, all complete, ten more: the second ten reuse the events of the first
        FakeGate g;
        int rc = 0;
        size_t max_inflight = 0;
        for (int round = 0; round < 2; ++round) {
            for (int i = 0; i < 10 && !rc; ++i) {
                rc = admit(g, 1, 20);
                max_inflight = std::max(max_inflight, g.inflight[0].size());
            }
            for (FakeEvents::Launch& l : g.events.launches) l.done.store(true);
        }
        printf("event_reuse: rc=%d events=%zu max_inflight=%zu\n", rc, g.events.bound.size(), max_inflight);
    }
    {
        // four host threads, a stream each; a launch "runs" until its thread says it has finished
        FakeGate g;
        g.events.wait_completes = false;
        std::atomic<int> failed{0};
        size_t max_inflight = 0;    // under the gate's lock
        auto work = [&](int stream) {
            std::mt19937 rng(stream);
            for (int i = 0; i < 200; ++i) {
                const int cus = 1 + (int)(rng() % 160);     // some pairs fit the device, some do not
                FakeEvents::Launch* mine = nullptr;
                const int rc = g.admit_and_launch(0, stream, cus, 256, [&]() {
                    mine = g.events.launch(stream, cus, 256);
                    max_inflight = std::max(max_inflight, g.inflight[0].size() + 1);
                    return 0;
                });
                if (rc) ++failed;
                for (unsigned spin = rng() % 8; spin; --spin) std::this_thread::yield();    // the launch "runs"
                if (mine) mine->done.store(true);
            }
        };
        std::vector<std::thread> threads;
        for (int s = 1; s <= 4; ++s) threads.emplace_back(work, s);
        for (std::thread& t : threads) t.join();
        printf("threads: failed=%d launches=%zu violations=%d events=%zu max_inflight=%zu waits=%zu\n", failed.load(),
               g.events.launches.size(), g.events.violations, g.events.bound.size(), max_inflight, g.events.waited.size());
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 6 && !strcmp(argv[1], "session")) return session(argv + 2);
    if (argc == 4 && !strcmp(argv[1], "hammer")) return hammer(argv[2], argv[3]);
    if (argc == 2 && !strcmp(argv[1], "gate")) return gate();
    if (argc == 2 && !strcmp(argv[1], "defaults")) {
        const ShareConfig& c = device_share().cfg;
        for (const std::string& d : c.lease_dirs) printf("%s ", c.lock_path(d, "KEY").c_str());
        printf("%s/%sPID %g %g %g\n", c.marker_dir.c_str(), c.marker_prefix("KEY").c_str(), c.lease_wait_s, c.user_active_s, c.marker_stale_s);
        return 0;
    }
    fprintf(stderr, "usage: device_share_check session DIR1 DIR2 MARKER_DIR WAIT_S | hammer DIR FILE | gate | defaults\n");
    return 2;
}
