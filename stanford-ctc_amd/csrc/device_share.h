// Co-residency guards: what keeps a persistent grid's workgroups resident when the GPU is not ours alone.
// Host code only (C++17 and POSIX, no GPU runtime): tests/device_share_check.cpp runs all of it on a CPU.
//
// Persistent kernels spin on other workgroups: every workgroup of the grid must be resident at
// once.  Three things can break that, each with its own guard:
//  (1) the grid does not fit the device at all (occupancy x CUs < grid): checked per (device,
//      kernel) before the launch (prepare_kernel, recurrent kernels' launcher) -> the per-step fallback
//      runs instead;
//  (2) ANOTHER PROCESS launches a persistent grid on the same device at the same time (two ranks
//      sharing one GPU): both get part of the CUs and spin forever.  "Shared-device mode" takes an
//      inter-process lease -- flock() on a per-device file in /dev/shm -- around every persistent
//      launch: stream drained, lock, launch, wait, unlock.  It is on when SCTC_SHARED_DEVICE=1
//      (the Python mirror sets it when the local ranks outnumber the visible devices) and turns
//      itself on for the rest of the process the first time a launch times out; the normal
//      one-rank-per-GPU path pays nothing;
//  (3) another STREAM of this process does the same (one-utterance-per-stream): the in-process
//      gate below admits a persistent launch only while the CUs of all persistent launches in
//      flight on other streams, plus its own, fit the device; otherwise it first waits (on the
//      host) for the oldest of them.
// What still gets through (CU masks the runtime does not report, a foreign persistent kernel of
// some other library) ends in the bounded spin -> SCTC_ERR_TIMEOUT -> the engine retries the step
// on the fallback.
//
// The files are a protocol between processes that may run different builds of the library:
// names, open flags, modes and time constants below change only together with every user of the directory.
#pragma once
#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include <dirent.h>
#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/file.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

namespace sctc {

// "0000:c1:00.0" -> "0000_c1_00_0": the device's part of every file name below
inline std::string share_key(const char* pci_bus_id)
{
    std::string key = pci_bus_id && *pci_bus_id ? pci_bus_id : "unknown";
    for (char& c : key)
        if (c == ':' || c == '.' || c == '/') c = '_';
    return key;
}

struct ShareConfig {
    std::vector<std::string> lease_dirs = {"/dev/shm", "/tmp"};    // tried in this order
    std::string marker_dir = "/dev/shm";
    double lease_wait_s = 30.0;
    double user_active_s = 0.3;     // a marker untouched for this long belongs to an idle process (a trainer launches every few ms)
    double marker_stale_s = 2.0;    // an UNLOCKED marker older than this is a dead process's

    std::string lock_path(const std::string& dir, const std::string& key) const { return dir + "/sctc_gpu_" + key + ".lock"; }
    std::string marker_prefix(const std::string& key) const { return "sctc_gpu_" + key + ".user."; }
};

// the name is predictable and the directory world-writable: never follow a planted symlink, never touch the mode of
// anything but a regular file of our own.  The process umask is left alone (another thread creating a file at that
// moment would inherit a cleared one): the mode is widened on the DESCRIPTOR.
inline int open_shared_file(const std::string& path, struct stat* st)
{
    const int fd = open(path.c_str(), O_CREAT | O_RDWR | O_CLOEXEC | O_NOFOLLOW, 0666);
    if (fd >= 0 && (fstat(fd, st) != 0 || !S_ISREG(st->st_mode))) { close(fd); return -1; }
    return fd;
}
inline void widen_own_file(int fd, const struct stat& st)
{
    if (st.st_uid == geteuid() && (st.st_mode & 0666) != 0666) (void)fchmod(fd, 0666);
}

inline double monotonic_s()
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

// Shared-device mode of the process.  SCTC_SHARED_DEVICE is read once, at the first touch, get or set alike; when
// it was there, the automatic switch (DeviceUsers) stays off whatever is set later.
class SharedMode {
    std::once_flag once;
    std::atomic<int> mode{0};
    bool named = false;
    void touch()
    {
        std::call_once(once, [this]() {
            const char* e = getenv("SCTC_SHARED_DEVICE");
            named = e != nullptr;
            mode.store((e && atoi(e) != 0) ? 1 : 0, std::memory_order_relaxed);
        });
    }

public:
    int get() { touch(); return mode.load(std::memory_order_relaxed); }
    void set(int on) { touch(); mode.store(on ? 1 : 0, std::memory_order_relaxed); }
    bool env_named() { touch(); return named; }
};

struct DeviceLease {      // inter-process: one lock file per physical device
    const ShareConfig& cfg;
    std::mutex mu;                       // serialises the threads of this process (flock is per open file)
    std::map<std::string, int> fds;      // a failed open is remembered too
    explicit DeviceLease(const ShareConfig& c) : cfg(c) {}
    int fd_for(const std::string& key)
    {
        auto it = fds.find(key);
        if (it != fds.end()) return it->second;
        int fd = -1;
        for (size_t k = 0; k < cfg.lease_dirs.size() && fd < 0; ++k) {
            struct stat st;
            fd = open_shared_file(cfg.lock_path(cfg.lease_dirs[k], key), &st);
            if (fd >= 0) widen_own_file(fd, st);
        }
        fds[key] = fd;
        return fd;
    }
};

struct LeaseGuard {
    DeviceLease& lease;
    int fd = -1;
    bool locked = false;
    LeaseGuard(DeviceLease& l, const std::string& key) : lease(l)
    {
        lease.mu.lock();
        fd = lease.fd_for(key);
        if (fd >= 0) {
            // bounded: another user holding the lock for good must not hang this process with its
            // mutex held -- after lease_wait_s the caller runs the step on the per-step fallback
            // Polling with a growing back-off (200 us .. 5 ms) instead of a blocking flock: the wait must end, and a
            // waiter that polls every 200 us re-acquires ahead of one that slept longer -- so every rank backs off the
            // same way.
            const double t0 = monotonic_s();
            useconds_t nap = 200;
            for (;;) {
                const int rc = flock(fd, LOCK_EX | LOCK_NB);
                if (rc == 0) { locked = true; break; }
                if (errno != EWOULDBLOCK && errno != EINTR) break;
                if (monotonic_s() - t0 > lease.cfg.lease_wait_s) {
                    // not silent: the step falls back to one launch per time step
                    fprintf(stderr, "sctc: device lease not obtained within %.0f s (another process holds %s): this step "
                                    "runs on the per-step recurrent kernels\n", lease.cfg.lease_wait_s, "the GPU's persistent-launch lock");
                    break;
                }
                usleep(nap);
                if (nap < 5000) nap += nap / 2;
            }
        }
    }
    ~LeaseGuard()
    {
        if (locked) (void)flock(fd, LOCK_UN);
        lease.mu.unlock();
    }
    LeaseGuard(const LeaseGuard&) = delete;
    LeaseGuard& operator=(const LeaseGuard&) = delete;
};

// Who else uses this PHYSICAL device?  Every process that launches a persistent grid keeps an
// exclusively flock'ed marker file /dev/shm/sctc_gpu_<pci-bus-id>.user.<pid> for its lifetime and touches it
// at every persistent launch; counting the markers that are locked AND fresh tells how many processes are
// launching persistent grids on the GPU right now,
// whatever HIP_VISIBLE_DEVICES / LOCAL_WORLD_SIZE / device ordinals look like (guessing from
// LOCAL_WORLD_SIZE > visible devices is wrong on an 8-GPU node whose launcher shows every rank one
// device, and wrong the other way on a box that exports a global visibility mask).  More than one ->
// shared-device mode switches itself on (one line on stderr).  Checked at persistent launches number
// 1, 2, 4, ... 32 and every 32nd after that (a directory scan of /dev/shm, ~20 us) while the mode is
// off; ranks that exchange their bus ids over a process group (dist_sgd.DataParallel) decide at once.
struct DeviceUsers {
    struct Mine { int fd = -1; unsigned launches = 0; };    // held marker, persistent launches so far
    const ShareConfig& cfg;
    std::mutex mu;
    std::map<std::string, Mine> mine;
    explicit DeviceUsers(const ShareConfig& c) : cfg(c) {}

    static double age_s(const struct stat& st)
    {
        struct timespec now;
        clock_gettime(CLOCK_REALTIME, &now);
        return (double)(now.tv_sec - st.st_mtim.tv_sec) + 1e-9 * (double)(now.tv_nsec - st.st_mtim.tv_nsec);
    }
    bool held_by_somebody(const std::string& path) const
    {
        const int fd = open(path.c_str(), O_RDWR | O_CLOEXEC | O_NOFOLLOW);
        if (fd < 0) return false;
        struct stat st;
        bool held = false;
        if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode)) {
            if (flock(fd, LOCK_SH | LOCK_NB) != 0) {
                // alive -- and ACTIVE: its owner touches the marker at every persistent launch; a process
                // that merely still exists (a test driver waiting for its child, an idle notebook) is no
                // reason to serialise launches
                const int err = errno;
                held = err == EWOULDBLOCK && age_s(st) < cfg.user_active_s;
            } else {
                // unlocked: its owner is gone -- or has created it a moment ago and not locked it yet (create and
                // lock are two calls): only a marker that has been lying there for a while is removed
                if (age_s(st) > cfg.marker_stale_s) (void)unlink(path.c_str());
                (void)flock(fd, LOCK_UN);
            }
        }
        close(fd);
        return held;
    }
    std::string own_marker(const std::string& key) const { return cfg.marker_prefix(key) + std::to_string((long)getpid()); }
    // number of live processes (this one included) that registered for device `key`; 0: no markers to be had
    int count(const std::string& key)
    {
        std::lock_guard<std::mutex> lock(mu);
        Mine& m = mine[key];
        const std::string prefix = cfg.marker_prefix(key), own = own_marker(key);
        if (m.fd < 0) {
            // (re)create the marker: a failed attempt -- or a marker a scanner removed between our open() and
            // flock() -- is tried again at the next check instead of leaving this process invisible for good
            const std::string path = cfg.marker_dir + "/" + own;
            struct stat st, on_disk;
            int fd = open_shared_file(path, &st);
            if (fd >= 0 && (flock(fd, LOCK_EX | LOCK_NB) != 0 || stat(path.c_str(), &on_disk) != 0 || on_disk.st_ino != st.st_ino)) {
                close(fd);      // not lockable, or the name no longer leads to the file we hold
                fd = -1;
            }
            if (fd >= 0) widen_own_file(fd, st);
            m.fd = fd;
        }
        if (m.fd < 0) return 0;
        int n = 1;
        if (DIR* d = opendir(cfg.marker_dir.c_str())) {
            while (struct dirent* e = readdir(d)) {
                if (strncmp(e->d_name, prefix.c_str(), prefix.size()) != 0 || own == e->d_name) continue;
                if (held_by_somebody(cfg.marker_dir + "/" + e->d_name)) ++n;
            }
            closedir(d);
        }
        return n;
    }
    // one persistent launch: the own marker says "active now"; true when this launch is one that scans
    bool due(const std::string& key)
    {
        std::lock_guard<std::mutex> lock(mu);
        Mine& m = mine[key];
        if (m.fd >= 0) (void)futimens(m.fd, nullptr);
        const unsigned k = ++m.launches;
        return k <= 32 ? (k & (k - 1)) == 0 : (k & 31) == 0;
    }
};

// The inter-process half as one object: the library has one (device_share()), a test builds its own in a
// temporary directory.
struct DeviceShare {
    ShareConfig cfg;
    SharedMode mode;
    DeviceLease lease{cfg};
    DeviceUsers users{cfg};
    DeviceShare() = default;
    explicit DeviceShare(const ShareConfig& c) : cfg(c) {}

    // one persistent launch on device `key`: is it to run under the lease?  While the mode is off and the
    // environment did not name it, the launches that are due look for other processes on the device.
    bool shared_for_launch(const std::string& key)
    {
        if (!mode.get() && !mode.env_named() && users.due(key)) {
            const int n = users.count(key);
            if (n > 1) {
                mode.set(1);
                fprintf(stderr, "sctc: %d processes run persistent kernels on this GPU: shared-device mode on "
                                "(their launches take turns under /dev/shm/sctc_gpu_*.lock)\n", n);
            }
        }
        return mode.get() != 0;
    }
};
inline DeviceShare& device_share()
{
    static DeviceShare share;
    return share;
}

// In-process: persistent launches in flight, per device.  `Events` supplies the four event operations --
//   bool done(Event)            has everything recorded before the event finished?
//   int  wait(Event)            blocks the host until it has; 0 or an error code
//   int  create(Event*)         0 or an error code
//   int  record(Event, Stream)  0 or an error code
// -- so that the admission loop runs unchanged over the GPU runtime's events and over a test's.
template <class Events>
struct PersistentGate {
    using Event = typename Events::Event;
    using Stream = typename Events::Stream;
    struct Entry { Event ev; Stream stream; int cus; };
    Events events;
    std::mutex mu;
    std::map<int, std::vector<Entry>> inflight;
    std::vector<Event> pool;

    // Waits (on the host) until `cus` more compute units' worth of persistent workgroups fit next to
    // what other streams have in flight, then launches and registers the launch's event -- all under
    // ONE lock: two host threads on different streams cannot both see an empty device and both
    // launch a whole-device grid (check-then-act race of a separate admit() / launched() pair).
    // `launch` returns 0 or an error code, which is returned with nothing registered.
    template <typename Launch>
    int admit_and_launch(int dev, Stream stream, int cus, int device_cus, Launch launch)
    {
        std::lock_guard<std::mutex> lock(mu);
        std::vector<Entry>& v = inflight[dev];
        for (;;) {
            int other = 0;
            for (size_t i = 0; i < v.size();) {
                if (events.done(v[i].ev)) {
                    pool.push_back(v[i].ev);
                    v.erase(v.begin() + i);
                    continue;
                }
                if (v[i].stream != stream) other += v[i].cus;   // same stream: serialised anyway
                ++i;
            }
            if (other == 0 || other + cus <= device_cus) break;
            for (size_t i = 0; i < v.size(); ++i)
                if (v[i].stream != stream) {
                    if (const int rc = events.wait(v[i].ev)) return rc;
                    break;
                }
        }
        if (const int rc = launch()) return rc;
        Event ev;
        if (!pool.empty()) { ev = pool.back(); pool.pop_back(); }
        else if (const int rc = events.create(&ev)) return rc;
        if (const int rc = events.record(ev, stream)) return rc;
        v.push_back(Entry{ev, stream, cus});
        return 0;
    }
};

}  // namespace sctc
