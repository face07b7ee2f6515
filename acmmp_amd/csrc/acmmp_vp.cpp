// acmmp_vp.cpp — view-parallel multi-GPU pass driver in C++,
// `acmmp_main <dense> --view_parallel`: one process per GPU, the views of
// every pass sharded over the ranks, depth maps exchanged with ONE RCCL
// all-gather per pass. The same schedule as the Python driver
// (acmmp_amd/distributed.py), so the .dmb outputs are bit-identical to it:
//
//   * sharding: LPT on W*H*(N-1) of the full-size reference image (the
//     placement, the band rows and the all-gather slots: acmmp_vp_plan.h);
//   * per scale (src/main_ACMMP.cpp:96-176): the images every owned view
//     needs are decoded once (acmmp_load_view) and kept in HBM; the first
//     scale runs the photometric + planar-prior pass, finer scales JBU +
//     the hierarchy pass; then two geometric passes; with -p the first
//     pass of the first scale is seeded from the prior PNGs (pSampler,
//     src/acmmp_definitions.cpp:99-177): the decoded 16-bit maps are uploaded
//     and the planes built on the device (acmmp_seed_planes_device);
//   * per view: the engine borrows the resident images
//     (acmmp_set_images_device), the gathered depth maps and the view's
//     previous state (acmmp_set_depth_maps_device /
//     acmmp_set_plane_hypotheses_device) and exports its results
//     device-to-device (acmmp_export_results); two engines per GPU, each
//     on its own HIP stream, take views off a shared queue;
//   * tail split: the V mod world cheapest views run on ALL ranks as row
//     bands (acmmp_run_patchmatch_band, 23-row halos all-gathered after
//     every half-sweep, bands all-gathered afterwards; bit-exact), each with
//     an owner rank that decodes, gathers and writes it (--no_split_tail
//     turns it off);
//   * exchange: the depth maps of a pass go through a padded
//     [world * slots, Hmax, Wmax] all-gather (ncclAllGather over xGMI, RCCL
//     has no all-gatherv). Jacobi order: every view of a pass reads the
//     previous pass's maps (the reference's second geometric pass is
//     Gauss-Seidel, src/main_ACMMP.cpp:159-172; acmmp_main without
//     --view_parallel keeps that order).
//
// Rendezvous: RANK / WORLD_SIZE / LOCAL_RANK / MASTER_ADDR from the
// environment (torchrun --no-python sets them); the ranks meet on TCP port
// ACMMP_RDZV_PORT (default MASTER_PORT + 1, torchrun's own store holds
// MASTER_PORT), where rank 0 hands out the ncclUniqueId. `--exchange tcp`
// all-gathers through that socket instead (host staging: several ranks on
// one GPU, where RCCL refuses duplicate devices — the 1-GPU parity tests).
#include <arpa/inet.h>
#include <netdb.h>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <poll.h>
#include <sys/socket.h>
#include <sys/stat.h>
#include <sys/time.h>
#include <unistd.h>

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cerrno>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/acmmp.h"
#include "acmmp_dense.h"
#include "acmmp_hostio.h"
#include "acmmp_vp.h"
#include "acmmp_vp_plan.h"

namespace {

using namespace acmmp_dense;
using namespace acmmp_vp;

struct Fail : std::runtime_error {
    using std::runtime_error::runtime_error;
};

[[noreturn]] void fail(const std::string &what) { throw Fail(what); }

void hip_check(hipError_t e, const char *what) {
    if (e != hipSuccess) fail(std::string(what) + ": " + hipGetErrorString(e));
}

void acmmp_check(int rc, const char *what, const acmmp_ctx *ctx = nullptr) {
    if (rc != ACMMP_OK)
        fail(std::string(what) + " failed (status " + std::to_string(rc) + ")" +
             (ctx ? std::string(": ") + acmmp_last_error(ctx) : std::string()));
}

// ------------------------------------------------------------ rendezvous
// Rank 0 accepts world - 1 connections; each client announces its rank. The
// sockets stay open for the id broadcast, barriers and the TCP exchange.
void send_all(int fd, const void *p, size_t n) {
    const char *c = static_cast<const char *>(p);
    while (n) {
        const ssize_t k = ::send(fd, c, n, MSG_NOSIGNAL);
        if (k <= 0) fail("rendezvous send failed");
        c += k;
        n -= (size_t)k;
    }
}

void recv_all(int fd, void *p, size_t n) {
    char *c = static_cast<char *>(p);
    while (n) {
        const ssize_t k = ::recv(fd, c, n, 0);
        if (k < 0 && (errno == EAGAIN || errno == EWOULDBLOCK))
            fail("exchange: no data from a peer within ACMMP_EXCHANGE_TIMEOUT (a rank failed or hangs)");
        if (k <= 0) fail("rendezvous recv failed (peer gone)");
        c += k;
        n -= (size_t)k;
    }
}

// Seconds a rank waits for its peers in one exchange step (a pass's
// slowest rank included) before it gives up: ACMMP_EXCHANGE_TIMEOUT, 1800.
int exchange_timeout_s() {
    const char *to = std::getenv("ACMMP_EXCHANGE_TIMEOUT");
    const int s = to && *to ? std::atoi(to) : 1800;
    return s > 0 ? s : 1800;
}

void set_socket_timeout(int fd, int seconds) {
    timeval tv{};
    tv.tv_sec = seconds;
    ::setsockopt(fd, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof tv);
    ::setsockopt(fd, SOL_SOCKET, SO_SNDTIMEO, &tv, sizeof tv);
}

class Group {
  public:
    int rank = 0, world = 1;

    Group(int rank_, int world_, const std::string &addr, int port) : rank(rank_), world(world_) {
        if (world == 1) return;
        if (rank == 0) {
            const int ls = ::socket(AF_INET, SOCK_STREAM, 0);
            const int one = 1;
            ::setsockopt(ls, SOL_SOCKET, SO_REUSEADDR, &one, sizeof one);
            sockaddr_in a{};
            a.sin_family = AF_INET;
            a.sin_port = htons((uint16_t)port);
            a.sin_addr.s_addr = htonl(INADDR_ANY);
            if (::bind(ls, (sockaddr *)&a, sizeof a) || ::listen(ls, world))
                fail("rendezvous: cannot listen on port " + std::to_string(port));
            peers_.assign(world, -1);
            const char *to = std::getenv("ACMMP_RDZV_TIMEOUT");  // seconds for every rank to arrive
            const int timeout_ms = 1000 * (to && *to ? std::atoi(to) : 600);
            for (int k = 1; k < world; ++k) {
                pollfd pf{ls, POLLIN, 0};
                if (::poll(&pf, 1, timeout_ms) != 1) {
                    ::close(ls);
                    fail("rendezvous: " + std::to_string(world - k) + " rank(s) did not connect to port " +
                         std::to_string(port) + " in time");
                }
                const int fd = ::accept(ls, nullptr, nullptr);
                if (fd < 0) fail("rendezvous accept failed");
                ::setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof one);
                set_socket_timeout(fd, std::max(1, timeout_ms / 1000));  // the announcement
                int32_t r = -1;
                recv_all(fd, &r, sizeof r);
                if (r <= 0 || r >= world || peers_[r] >= 0) fail("rendezvous: bad rank announcement");
                peers_[r] = fd;
            }
            ::close(ls);
            for (int k = 1; k < world; ++k) set_socket_timeout(peers_[k], exchange_timeout_s());
        } else {
            addrinfo hints{}, *res = nullptr;
            hints.ai_family = AF_INET;
            hints.ai_socktype = SOCK_STREAM;
            if (::getaddrinfo(addr.c_str(), std::to_string(port).c_str(), &hints, &res) || !res)
                fail("rendezvous: cannot resolve " + addr);
            int fd = -1;
            for (int attempt = 0; attempt < 600 && fd < 0; ++attempt) {  // rank 0 may start later: retry 60 s
                fd = ::socket(AF_INET, SOCK_STREAM, 0);
                if (::connect(fd, res->ai_addr, res->ai_addrlen)) {
                    ::close(fd);
                    fd = -1;
                    ::usleep(100000);
                }
            }
            ::freeaddrinfo(res);
            if (fd < 0) fail("rendezvous: cannot connect to " + addr + ":" + std::to_string(port));
            const int one = 1;
            ::setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof one);
            set_socket_timeout(fd, exchange_timeout_s());
            const int32_t r = rank;
            send_all(fd, &r, sizeof r);
            root_ = fd;
        }
    }

    ~Group() {
        for (int fd : peers_)
            if (fd >= 0) ::close(fd);
        if (root_ >= 0) ::close(root_);
    }

    // rank 0's bytes to every rank
    void broadcast(void *p, size_t n) {
        if (world == 1) return;
        if (rank == 0)
            for (int k = 1; k < world; ++k) send_all(peers_[k], p, n);
        else
            recv_all(root_, p, n);
    }

    // every rank's n bytes, concatenated in rank order, to every rank
    void allgather(const void *mine, void *all, size_t n) {
        char *out = static_cast<char *>(all);
        std::memcpy(out + (size_t)rank * n, mine, n);
        if (world == 1) return;
        if (rank == 0) {
            for (int k = 1; k < world; ++k) recv_all(peers_[k], out + (size_t)k * n, n);
            for (int k = 1; k < world; ++k) send_all(peers_[k], out, (size_t)world * n);
        } else {
            send_all(root_, mine, n);
            recv_all(root_, out, (size_t)world * n);
        }
    }

    void barrier() {
        char b = 0;
        std::vector<char> all((size_t)world);
        allgather(&b, all.data(), 1);
    }

  private:
    std::vector<int> peers_;
    int root_ = -1;
};

// ------------------------------------------------------------ exchange
class Exchange {
  public:
    Exchange(Group &g, bool rccl, int device) : g_(g), rccl_(rccl) {
        const auto t0 = std::chrono::steady_clock::now();
        hip_check(hipSetDevice(device), "hipSetDevice");
        hip_check(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking), "hipStreamCreate");
        if (rccl_) {
            ncclUniqueId id;
            if (g.rank == 0 && ncclGetUniqueId(&id) != ncclSuccess) fail("ncclGetUniqueId failed");
            g.broadcast(&id, sizeof id);
            const ncclResult_t r = ncclCommInitRank(&comm_, g.world, id, g.rank);
            if (r != ncclSuccess) fail(std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
        }
        if (std::getenv("ACMMP_HOST_TIMING"))
            std::fprintf(stderr, "[rank %d] exchange init (%s)=%.2fs\n", g.rank, rccl_ ? "rccl" : "local/tcp",
                         std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    }
    ~Exchange() {
        if (comm_) ncclCommDestroy(comm_);
        if (stream_) (void)hipStreamDestroy(stream_);
    }

    // d_recv[world * count] = concatenation of every rank's d_send[count]
    void allgather(const float *d_send, float *d_recv, size_t count) {
        if (rccl_) {  // world 1 included: the same RCCL call as at 8 GPUs
            const ncclResult_t r = ncclAllGather(d_send, d_recv, count, ncclFloat32, comm_, stream_);
            if (r != ncclSuccess) fail(std::string("ncclAllGather: ") + ncclGetErrorString(r));
            wait_rccl();
            return;
        } else if (g_.world == 1) {
            hip_check(hipMemcpyAsync(d_recv, d_send, count * sizeof(float), hipMemcpyDeviceToDevice, stream_),
                      "hipMemcpyAsync");
        } else {
            std::vector<float> mine(count), all(count * (size_t)g_.world);
            hip_check(hipMemcpy(mine.data(), d_send, count * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy");
            g_.allgather(mine.data(), all.data(), count * sizeof(float));
            hip_check(hipMemcpy(d_recv, all.data(), all.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy");
        }
        // the engines' streams do not wait on this one
        hip_check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
    }

  private:
    // the all-gather has finished, or the communicator reported an error /
    // the peers did not arrive within ACMMP_EXCHANGE_TIMEOUT: then abort it
    // (the peers' collectives fail too) and exit non-zero instead of blocking
    void wait_rccl() {
        const auto deadline = std::chrono::steady_clock::now() + std::chrono::seconds(exchange_timeout_s());
        for (;;) {
            const hipError_t q = hipStreamQuery(stream_);
            if (q == hipSuccess) return;
            if (q != hipErrorNotReady) hip_check(q, "ncclAllGather stream");
            ncclResult_t async = ncclSuccess;
            if (ncclCommGetAsyncError(comm_, &async) != ncclSuccess || async != ncclSuccess) {
                abort_comm();
                fail(std::string("ncclAllGather: ") + ncclGetErrorString(async));
            }
            if (std::chrono::steady_clock::now() > deadline) {
                abort_comm();
                fail("ncclAllGather: peers did not arrive within ACMMP_EXCHANGE_TIMEOUT");
            }
            std::this_thread::sleep_for(std::chrono::microseconds(50));
        }
    }
    void abort_comm() {
        (void)ncclCommAbort(comm_);
        comm_ = nullptr;
    }

    Group &g_;
    bool rccl_;
    ncclComm_t comm_ = nullptr;
    hipStream_t stream_ = nullptr;
};

// ------------------------------------------------------------ buffers
struct DevBuf {
    float *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    explicit DevBuf(size_t count) : n(count) {
        if (count) hip_check(hipMalloc((void **)&p, count * sizeof(float)), "hipMalloc");
    }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        std::swap(p, o.p);
        std::swap(n, o.n);
        return *this;
    }
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

struct ViewState {
    DevBuf planes, costs;  // (H, W, 4) world normal + depth, (H, W)
    DevBuf depth;          // (H, W): the planes' depth channel, what the next pass's gather and JBU read
    int W = 0, H = 0;
    DevBuf jbu;  // upsampled depth of the hierarchy pass (device, the next scale's W x H)
    ViewState() = default;
    ViewState(int w, int h) : planes((size_t)w * h * 4), costs((size_t)w * h), depth((size_t)w * h), W(w), H(h) {}
};

// Rows [lo, hi) of a device map of `row_floats` floats per row, to (pack) or
// from a contiguous block, on `cs`.
void copy_rows(void *map, size_t row_floats, int lo, int hi, float *block, bool pack, hipStream_t cs) {
    const size_t n = (size_t)(hi - lo) * row_floats;
    if (!n) return;
    float *rows = static_cast<float *>(map) + (size_t)lo * row_floats;
    hip_check(hipMemcpyAsync(pack ? block : rows, pack ? rows : block, n * sizeof(float), hipMemcpyDeviceToDevice, cs),
              "hipMemcpyAsync");
}

// One padded all-gather of a map per view (acmmp_vp_plan.h's GatherLayout):
// the zero-filled send buffer with this rank's views in its slots, and the
// gathered buffer every view's map is borrowed from in place.
class PaddedGather {
  public:
    PaddedGather() = default;
    PaddedGather(const Plan &plan, int hmax, int wmax)
        : at_{&plan, hmax, wmax}, send_(at_.send_floats()), recv_(at_.recv_floats()) {
        hip_check(hipMemset(send_.p, 0, send_.n * sizeof(float)), "hipMemset");
    }
    // view v (one of this rank's) = the contiguous w x h device map
    void put(int v, const float *map, int w, int h) {
        hip_check(hipMemcpy2D(send_.p + at_.send_offset(v), (size_t)at_.wmax * sizeof(float), map,
                              (size_t)w * sizeof(float), (size_t)w * sizeof(float), (size_t)h,
                              hipMemcpyDeviceToDevice),
                  "hipMemcpy2D");
    }
    // every rank's views on every rank (the puts above are complete first)
    void gather(Exchange &ex) {
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        ex.allgather(send_.p, recv_.p, send_.n);
    }
    void drop_send() { send_ = DevBuf(); }  // nothing more is put in
    // view v's gathered map, rows pitch() floats apart
    const float *map(int v) const { return recv_.p + at_.recv_offset(v); }
    int pitch() const { return at_.wmax; }

  private:
    GatherLayout at_;
    DevBuf send_, recv_;
};

// One pass of the schedule over every view (src/main_ACMMP.cpp:96-176)
struct Pass {
    bool geom, planar, hier, multi;
    bool seeded = false;  // -p: the first scale's first pass starts from the prior planes (:107-120)
    // the first scale: photometric, then again with the planar prior (:109-120)
    static Pass planar_prior() { return {false, true, false, false}; }
    // a finer scale, after JBU: the same from the upsampled previous scale (:146-155)
    static Pass hierarchy() { return {false, true, true, false}; }
    // geometric consistency; every one after a scale's first is multi-geometry (:121-138, :156-173)
    static Pass geometric(bool multi) { return {true, false, false, multi}; }
};

// --------------------------------------------------------------- driver
class Driver {
  public:
    Driver(const VpOptions &o, Group &g)
        : o_(o), g_(g), ex_(g, o.exchange_rccl, o.device), output_folder_(o.dense + o.output_dir) {
        read_problems();
        plan();
        create_engines();
    }

    ~Driver() {
        for (auto &t : writers_)
            if (t.joinable()) t.join();
        for (auto *e : engines_) acmmp_destroy(e);
        for (auto cs : copy_) (void)hipStreamDestroy(cs);
        for (auto &kv : textures_) acmmp_texture_destroy(kv.second);
    }

    void run() {
        ::mkdir(output_folder_.c_str(), 0777);
        bool first = true;
        while (max_down_ >= 0) {
            scale_step(problems_.data(), (int)problems_.size());
            {
                Clock c(this, "load");
                read_shapes();
                if (first) plan_.apply_halo_rule(height_);  // the coarsest scale decides which views stay split
                depths_ = PaddedGather(plan_, hmax_, wmax_);
                load_views();
            }
            if (first) {
                first = false;
                Pass pass = Pass::planar_prior();
                if (o_.prior) {
                    Clock c(this, "prior_load");
                    load_prior_maps();
                    pass.seeded = true;
                }
                run_pass(pass);
                prior_maps_.clear();  // only this pass is seeded
            } else {
                {
                    Clock c(this, "jbu");
                    jbu();
                }
                run_pass(Pass::hierarchy());
            }
            for (int gi = 0; gi < o_.geom_iterations; ++gi) run_pass(Pass::geometric(gi > 0));
            max_down_--;
        }
        {
            Clock c(this, "flush_writes");
            flush_writes();
        }
        g_.barrier();
        if (std::getenv("ACMMP_HOST_TIMING")) {
            std::fprintf(stderr, "[rank %d]", g_.rank);
            for (auto &kv : phase_s_) std::fprintf(stderr, " %s=%.2fs", kv.first.c_str(), kv.second);
            std::fprintf(stderr, "\n");
        }
    }

  private:
    struct Task {
        int view;  // problem index
        Pass pass;
    };

    void read_problems() {
        problems_.resize(4096);
        int n = 0;
        acmmp_check(acmmp_generate_sample_list(o_.dense.c_str(), problems_.data(), (int)problems_.size(), &n),
                    "GenerateSampleList");
        problems_.resize((size_t)n);
        acmmp_check(acmmp_compute_multiscale_settings(o_.dense.c_str(), problems_.data(), n, &max_down_),
                    "ComputeMultiScaleSettings");
        for (int i = 0; i < n; ++i) index_of_[problems_[(size_t)i].ref_image_id] = i;
        state_.resize((size_t)n);
    }

    // LPT on W*H*max(N-1, 1) of the full-size reference image
    void plan() {
        std::vector<double> cost;
        for (const acmmp_problem &p : problems_) {
            int w = 0, h = 0;
            acmmp_check(acmmp_view_size(o_.dense.c_str(), p.ref_image_id, 0, &w, &h), "image header");
            cost.push_back((double)w * h * std::max(p.num_src_images, 1));
        }
        plan_ = plan_views(cost, g_.world, o_.split_tail);
    }

    // two engines per GPU by default, each with a stream for the driver's own copies
    void create_engines() {
        for (int k = 0; k < std::max(o_.concurrent_views, 1); ++k) {
            acmmp_ctx *ctx = nullptr;
            acmmp_check(acmmp_create(o_.device, &ctx), "acmmp_create");
            engines_.push_back(ctx);
            hipStream_t cs = nullptr;
            hip_check(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking), "hipStreamCreate");
            copy_.push_back(cs);
        }
    }

    const std::vector<int> &owned() const { return plan_.owned(g_.rank); }
    // the views this rank computes: its own whole, then a band of every split one
    std::vector<int> computed() const {
        std::vector<int> views = plan_.mine(g_.rank);
        views.insert(views.end(), plan_.split.begin(), plan_.split.end());
        return views;
    }
    const acmmp_camera &ref_cam(int v) const { return cams_.at(problems_[(size_t)v].ref_image_id); }

    // wall seconds per phase (ACMMP_HOST_TIMING=1 prints them)
    struct Clock {
        Driver *d;
        const char *name;
        std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
        Clock(Driver *d_, const char *n) : d(d_), name(n) {}
        ~Clock() {
            d->phase_s_[name] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        }
    };

    // the .dmb writers of the previous pass have finished (they read the
    // state buffers the next pass end replaces); their first error is raised
    void flush_writes() {
        for (auto &t : writers_) t.join();
        writers_.clear();
        for (auto &e : write_errs_)
            if (!e.empty()) fail(e);
        write_errs_.clear();
    }

    // a pass's outputs written by 4 host threads while the next pass computes
    void start_writes(bool geom) {
        const int nw = (int)std::min<size_t>(4, owned().size());
        write_errs_.assign((size_t)nw, std::string());
        for (int w = 0; w < nw; ++w)
            writers_.emplace_back([this, w, nw, geom]() {
                try {
                    hip_check(hipSetDevice(o_.device), "hipSetDevice");
                    for (size_t k = (size_t)w; k < owned().size(); k += (size_t)nw)
                        write_outputs(owned()[k], state_[(size_t)owned()[k]], geom);
                } catch (const std::exception &e) {
                    write_errs_[(size_t)w] = e.what();
                }
            });
    }

    // Images of this scale, decoded once per node: every rank decodes the
    // reference images of ITS views (acmmp_load_view: JPEG decode + rescale,
    // InputInitialization src/ACMMP.cpp:536-598) and the images travel in
    // ONE padded all-gather, like the depth maps (RCCL over xGMI); cameras
    // come from the headers and cam files of every image a view needs.
    void load_views() {
        for (auto &kv : textures_) acmmp_texture_destroy(kv.second);
        textures_.clear();
        images_.clear();
        cams_.clear();
        const std::vector<int> &own = owned();
        std::vector<int> need;
        for (int v : computed()) {
            const acmmp_problem &p = problems_[(size_t)v];
            need.push_back(p.ref_image_id);
            for (int s = 0; s < p.num_src_images; ++s) need.push_back(p.src_image_ids[s]);
        }
        std::sort(need.begin(), need.end());
        need.erase(std::unique(need.begin(), need.end()), need.end());
        for (int id : need)
            if (!index_of_.count(id)) fail("source id " + std::to_string(id) + " is not a problem index");
        // work items: the cameras of every needed image, the pixels of my refs
        std::vector<acmmp_camera> cams(need.size());
        std::vector<std::vector<float>> host(own.size());
        std::vector<acmmp_camera> own_cams(own.size());
        const size_t nwork = need.size() + own.size();
        auto image_id = [&](size_t k) {
            return k < need.size() ? need[k] : problems_[(size_t)own[k - need.size()]].ref_image_id;
        };
        std::string err;
        const int load_rc = parallel_index(
            (int)nwork, acmmp_host_threads(),
            [&](int i) -> int {
                const size_t k = (size_t)i;
                const bool pixels = k >= need.size();
                const int id = image_id(k);
                acmmp_camera &cam = pixels ? own_cams[k - need.size()] : cams[k];
                const int size = problems_[(size_t)index_of_.at(id)].cur_image_size;
                const int rc = acmmp_load_view(o_.dense.c_str(), id, size, nullptr, 0, &cam);
                if (rc != ACMMP_OK && rc != ACMMP_ERR_ARG) return rc;
                if (!pixels) return ACMMP_OK;
                std::vector<float> &h = host[k - need.size()];
                h.resize((size_t)cam.width * cam.height);
                return acmmp_load_view(o_.dense.c_str(), id, size, h.data(), h.size(), &cam);
            },
            [&](int i) {
                return "view " + std::to_string(image_id((size_t)i)) + ": acmmp_load_view: " + acmmp_pipeline_last_error();
            },
            err);
        if (load_rc) fail(err);
        // my refs: kept contiguous for JBU, and padded into my all-gather slots
        gathered_images_ = PaddedGather(plan_, hmax_, wmax_);
        for (size_t k = 0; k < own.size(); ++k) {
            const acmmp_camera &c = own_cams[k];
            const int v = own[k];
            if (c.height != height_[(size_t)v] || c.width != width_[(size_t)v])
                fail("view " + std::to_string(problems_[(size_t)v].ref_image_id) + ": image size disagrees with its header");
            DevBuf d(host[k].size());
            hip_check(hipMemcpy(d.p, host[k].data(), host[k].size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy");
            gathered_images_.put(v, d.p, c.width, c.height);
            images_.emplace(problems_[(size_t)v].ref_image_id, std::move(d));
        }
        gathered_images_.gather(ex_);
        gathered_images_.drop_send();
        // the padded footprint records, built once per image and scale from
        // the gathered image (row pitch Wmax)
        for (size_t k = 0; k < need.size(); ++k) {
            const acmmp_camera &c = cams[k];
            acmmp_texture *t = nullptr;
            acmmp_check(acmmp_texture_create(o_.device, gathered_images_.map(index_of_.at(need[k])),
                                             gathered_images_.pitch(), c.width, c.height, &t),
                        "acmmp_texture_create");
            textures_[need[k]] = t;
            cams_[need[k]] = c;
        }
        // a split view's JBU runs on every rank: its reference image, unpadded
        for (int v : plan_.split) {
            const int id = problems_[(size_t)v].ref_image_id;
            if (images_.count(id)) continue;
            const acmmp_camera &c = cams_.at(id);
            DevBuf d((size_t)c.width * c.height);
            hip_check(hipMemcpy2DAsync(d.p, (size_t)c.width * sizeof(float), gathered_images_.map(v),
                                       (size_t)gathered_images_.pitch() * sizeof(float),
                                       (size_t)c.width * sizeof(float), (size_t)c.height, hipMemcpyDeviceToDevice,
                                       copy_[0]),
                      "hipMemcpy2DAsync");
            hip_check(hipStreamSynchronize(copy_[0]), "hipStreamSynchronize");
            images_.emplace(id, std::move(d));
        }
    }

    // -p: the decoded prior maps of every view this rank computes (a band of
    // a split view needs the view's whole seed: every rank reads it from the
    // dense folder), PNGs read on the loader pool, words uploaded as they are.
    // pSampler is asked for camera `problem index` (src/acmmp_definitions.cpp:277).
    struct PriorMapsDev {
        DevBuf depth, normals;  // uint16 words (acmmp_hostio::PriorMaps' layout)
        int dw = 0, dh = 0, dc = 0, nw = 0, nh = 0;
    };
    void load_prior_maps() {
        const std::vector<int> views = computed();
        std::vector<acmmp_hostio::PriorMaps> host(views.size());
        std::vector<std::string> msg(views.size());
        std::string err;
        const int rc = parallel_index(
            (int)views.size(), acmmp_host_threads(),
            [&](int i) {
                const size_t k = (size_t)i;
                return acmmp_hostio::read_prior_maps(o_.dense, views[k], host[k], msg[k]);
            },
            [&](int i) { return msg[(size_t)i]; }, err);
        if (rc) fail(err);
        auto upload = [](const std::vector<uint16_t> &words) {
            DevBuf d((words.size() + 1) / 2);
            hip_check(hipMemcpy(d.p, words.data(), words.size() * sizeof(uint16_t), hipMemcpyHostToDevice),
                      "hipMemcpy");
            return d;
        };
        for (size_t k = 0; k < views.size(); ++k) {
            const acmmp_hostio::PriorMaps &m = host[k];
            PriorMapsDev d;
            d.depth = upload(m.depth);
            d.normals = upload(m.normals);
            d.dw = m.dw, d.dh = m.dh, d.dc = m.dc, d.nw = m.nw, d.nh = m.nh;
            prior_maps_[views[k]] = std::move(d);
        }
    }

    // The seeded pass's start planes of view t.view on an engine that holds
    // its images (GetPriorPlaneEstimate + SetPlanarPrior,
    // src/acmmp_definitions.cpp:275-281): built on `cs` at the view's size with
    // GetCamera(problem index) -- an index into the problem's own cameras,
    // camera 0 beyond them, as the reference -- and copied into the engine's
    // seed buffer. The engine reads the returned buffer on its stream: kept
    // until its run has been synchronised.
    DevBuf set_seed_prior(acmmp_ctx *eng, const Task &t, hipStream_t cs) {
        const acmmp_problem &pr = problems_[(size_t)t.view];
        const int k = t.view < 1 + pr.num_src_images ? t.view : 0;
        const acmmp_camera &cam = cams_.at(k == 0 ? pr.ref_image_id : pr.src_image_ids[k - 1]);
        const acmmp_camera &ref = ref_cam(t.view);
        const PriorMapsDev &m = prior_maps_.at(t.view);
        DevBuf planes((size_t)ref.width * ref.height * 4);
        const int rc = acmmp_seed_planes_device(o_.device, reinterpret_cast<const uint16_t *>(m.depth.p), m.dw, m.dh,
                                                m.dc, reinterpret_cast<const uint16_t *>(m.normals.p), m.nw, m.nh, &cam,
                                                ref.height, ref.width, planes.p, cs);
        if (rc)
            fail("view " + std::to_string(pr.ref_image_id) + ": acmmp_seed_planes_device: " +
                 acmmp_pipeline_last_error());
        acmmp_check(acmmp_wait_stream(eng, cs), "acmmp_wait_stream", eng);
        acmmp_check(acmmp_set_seed_prior_device(eng, planes.p), "acmmp_set_seed_prior_device", eng);
        return planes;
    }

    // height and width of every view at this scale
    void read_shapes() {
        height_.assign(problems_.size(), 0);
        width_.assign(problems_.size(), 0);
        hmax_ = wmax_ = 0;
        for (size_t i = 0; i < problems_.size(); ++i) {
            acmmp_check(acmmp_view_size(o_.dense.c_str(), problems_[i].ref_image_id, problems_[i].cur_image_size,
                                        &width_[i], &height_[i]),
                        "image header");
            hmax_ = std::max(hmax_, height_[i]);
            wmax_ = std::max(wmax_, width_[i]);
        }
    }

    acmmp_params view_params(int v, const Pass &pass) const {
        acmmp_params p;
        acmmp_default_params(&p);
        if (pass.geom) {  // SetGeomConsistencyParams (src/ACMMP.cpp:447-454)
            p.geom_consistency = 1;
            p.max_iterations = 2;
            if (pass.multi) p.multi_geometry = 1;
        }
        if (pass.hier) p.hierarchy = 1;
        p.seed_lo = o_.seed + (unsigned)problems_[(size_t)v].ref_image_id;
        p.seed_hi = (unsigned)pass_index_;
        if (o_.iterations > 0) p.max_iterations = o_.iterations;
        if (o_.patch_size) p.patch_size = o_.patch_size;
        if (o_.radius_increment) p.radius_increment = o_.radius_increment;
        return p;
    }

    // One view's inputs on an engine: parameters and textures, and for a
    // geometric pass the gathered depth maps of the previous pass (borrowed in
    // place) and the view's previous state.
    void set_view_inputs(acmmp_ctx *eng, const Task &t) {
        const acmmp_problem &pr = problems_[(size_t)t.view];
        std::vector<int> ids = {pr.ref_image_id};
        for (int s = 0; s < pr.num_src_images; ++s) ids.push_back(pr.src_image_ids[s]);
        std::vector<acmmp_camera> cams;
        std::vector<const acmmp_texture *> tex;
        for (int id : ids) {
            cams.push_back(cams_.at(id));
            tex.push_back(textures_.at(id));
        }
        const acmmp_params p = view_params(t.view, t.pass);
        acmmp_check(acmmp_set_params(eng, &p), "acmmp_set_params", eng);
        acmmp_check(acmmp_set_images_textures(eng, (int)ids.size(), cams.data(), tex.data(), 0),
                    "acmmp_set_images_textures", eng);
        if (!t.pass.geom) return;
        std::vector<const float *> deps;
        for (int id : ids) deps.push_back(depths_.map(index_of_.at(id)));
        const std::vector<int32_t> pitches(ids.size(), depths_.pitch());
        acmmp_check(acmmp_set_depth_maps_device(eng, deps.data(), pitches.data()), "acmmp_set_depth_maps_device", eng);
        const ViewState &prev = state_[(size_t)t.view];
        acmmp_check(acmmp_set_plane_hypotheses_device(eng, prev.planes.p, prev.costs.p),
                    "acmmp_set_plane_hypotheses_device", eng);
    }

    // The hierarchy pass's inputs of a W x H view from its previous scale:
    // scaled planes = that scale's normals + (costs, or the JBU depth when no
    // upsample). The engine borrows the returned buffer until its run has
    // been synchronised.
    DevBuf set_hierarchy_inputs(acmmp_ctx *eng, const ViewState &prev, int W, int H, hipStream_t cs) {
        const int sh = prev.H, sw = prev.W;
        const size_t S = (size_t)sh * sw;
        const bool upsample = sw != H || sh != W;  // src/ACMMP.cpp:766, rows/cols swap included
        if (!upsample && prev.jbu.n < S) fail("hierarchy input: JBU depth smaller than the scaled planes");
        DevBuf scaled(S * 4);
        // built on the device: the normals, then the 4th channel as a
        // strided copy (4 of every 16 bytes), as the Python driver does
        // (device-to-device hipMemcpy does not wait for the copy, and the
        // engine stream is non-blocking: copy on `cs` and wait for it)
        hip_check(hipMemcpyAsync(scaled.p, prev.planes.p, S * 4 * sizeof(float), hipMemcpyDeviceToDevice, cs),
                  "hipMemcpyAsync");
        hip_check(hipMemcpy2DAsync(scaled.p + 3, 4 * sizeof(float), upsample ? prev.costs.p : prev.jbu.p,
                                   sizeof(float), sizeof(float), S, hipMemcpyDeviceToDevice, cs),
                  "hipMemcpy2DAsync");
        hip_check(hipStreamSynchronize(cs), "hipStreamSynchronize");
        acmmp_check(acmmp_set_hierarchy_inputs_device(eng, scaled.p, sw, sh, prev.jbu.p),
                    "acmmp_set_hierarchy_inputs_device", eng);
        return scaled;
    }

    // One view of a pass on an engine, by `run` (run_whole, or run_band on
    // every rank at once): its inputs, then its new state.
    using Run = void (Driver::*)(acmmp_ctx *, const Pass &, ViewState &, hipStream_t);
    ViewState compute(acmmp_ctx *eng, const Task &t, hipStream_t cs, Run run) {
        set_view_inputs(eng, t);
        const acmmp_camera &c = ref_cam(t.view);
        DevBuf scaled, seed;
        if (t.pass.hier) scaled = set_hierarchy_inputs(eng, state_[(size_t)t.view], c.width, c.height, cs);
        if (t.pass.seeded) seed = set_seed_prior(eng, t, cs);
        ViewState out(c.width, c.height);
        (this->*run)(eng, t.pass, out, cs);
        return out;
    }

    // RunPatchMatch, twice with the planar prior between (src/acmmp_definitions.cpp:306-379)
    void run_whole(acmmp_ctx *eng, const Pass &pass, ViewState &out, hipStream_t) {
        acmmp_check(acmmp_run_patchmatch_async(eng), "acmmp_run_patchmatch_async", eng);
        if (pass.planar) {
            acmmp_check(acmmp_synchronize(eng), "acmmp_synchronize", eng);
            int nsp = 0, ntri = 0;
            acmmp_check(acmmp_prepare_planar_prior(eng, &nsp, &ntri), "acmmp_prepare_planar_prior", eng);
            acmmp_check(acmmp_run_patchmatch_async(eng), "acmmp_run_patchmatch_async", eng);
        }
        acmmp_check(acmmp_export_results(eng, out.planes.p, out.costs.p, out.depth.p), "acmmp_export_results", eng);
        acmmp_check(acmmp_synchronize(eng), "acmmp_synchronize", eng);
    }

    std::pair<int, int> band_rows(int H, int k) const { return acmmp_vp::band_rows(H, g_.world, k); }

    // The halo exchange of a band run (acmmp_run_patchmatch_band's callback):
    // each rank all-gathers [rows the band above reads | rows the band below
    // reads] of the colour just written (plane float4, cost, selected views),
    // then takes its neighbours' parts. One all-gather of 2 x 23 rows per
    // rank and half-sweep (RCCL over xGMI, or the TCP exchange).
    struct BandCtx {
        Driver *d;
        hipStream_t cs;
        DevBuf send, recv;
        std::string err;
    };
    static int band_exchange(void *user, const acmmp_band_halo *h) {
        BandCtx *b = static_cast<BandCtx *>(user);
        try {
            b->d->halo_exchange(*b, *h);
            return 0;
        } catch (const std::exception &e) {
            b->err = e.what();
            return 1;
        }
    }
    void halo_exchange(BandCtx &b, const acmmp_band_halo &h) {
        const size_t Wh = (size_t)h.Wh, K = ACMMP_BAND_HALO;
        const size_t part = K * Wh * 6;  // floats: K rows of plane (4) + cost + selected views
        if (b.send.n != 2 * part) {
            b.send = DevBuf(2 * part);
            b.recv = DevBuf(2 * part * (size_t)g_.world);
        }
        // the sweep that wrote these rows ran on the engine's stream
        hip_check(hipStreamSynchronize((hipStream_t)h.stream), "hipStreamSynchronize");
        // rows [lo, hi) of the three maps, to (pack) or from one part
        auto rows = [&](float *p, int lo, int hi, bool pack) {
            copy_rows(h.plane, Wh * 4, lo, hi, p, pack, b.cs);
            copy_rows(h.cost, Wh, lo, hi, p + K * Wh * 4, pack, b.cs);
            copy_rows(h.sv, Wh, lo, hi, p + K * Wh * 5, pack, b.cs);
        };
        rows(b.send.p, h.send_up_lo, h.send_up_hi, true);
        rows(b.send.p + part, h.send_down_lo, h.send_down_hi, true);
        hip_check(hipStreamSynchronize(b.cs), "hipStreamSynchronize");
        ex_.allgather(b.send.p, b.recv.p, b.send.n);
        const int r = g_.rank;
        if (r > 0) rows(b.recv.p + (size_t)(r - 1) * 2 * part + part, h.recv_up_lo, h.recv_up_hi, false);
        if (r + 1 < g_.world) rows(b.recv.p + (size_t)(r + 1) * 2 * part, h.recv_down_lo, h.recv_down_hi, false);
        // the engine's next sweep is enqueued after this returns
        hip_check(hipStreamSynchronize(b.cs), "hipStreamSynchronize");
    }

    // every band's rows of the exported (planes, costs) from its rank, on every rank
    void gather_bands(ViewState &out, hipStream_t cs) {
        const int W = out.W, H = out.H;
        int rmax = 0;
        for (int k = 0; k < g_.world; ++k) rmax = std::max(rmax, band_rows(H, k).second - band_rows(H, k).first);
        const size_t per = (size_t)rmax * W * 5;
        DevBuf send(per), recv(per * (size_t)g_.world);
        // band k's rows of both maps, to (pack) or from its rank's block
        auto band = [&](int k, float *block, bool pack) {
            const auto [lo, hi] = band_rows(H, k);
            copy_rows(out.planes.p, (size_t)W * 4, lo, hi, block, pack, cs);
            copy_rows(out.costs.p, (size_t)W, lo, hi, block + (size_t)rmax * W * 4, pack, cs);
        };
        band(g_.rank, send.p, true);
        hip_check(hipStreamSynchronize(cs), "hipStreamSynchronize");
        ex_.allgather(send.p, recv.p, per);
        for (int k = 0; k < g_.world; ++k)
            if (k != g_.rank) band(k, recv.p + (size_t)k * per, false);
        hip_check(hipStreamSynchronize(cs), "hipStreamSynchronize");
    }

    // the depth channel of the gathered planes (a band export has no whole depth map)
    void extract_depth(ViewState &s, hipStream_t cs) {
        hip_check(hipMemcpy2DAsync(s.depth.p, sizeof(float), s.planes.p + 3, 4 * sizeof(float), sizeof(float),
                                   (size_t)s.W * s.H, hipMemcpyDeviceToDevice, cs),
                  "hipMemcpy2DAsync");
        hip_check(hipStreamSynchronize(cs), "hipStreamSynchronize");
    }

    // One view's run split in row bands over every rank (the engine already
    // holds the view's inputs): this rank's band, the halos exchanged every
    // half-sweep, the bands gathered; with the planar prior, the prior is
    // rebuilt on every rank from the gathered first run, then the second run
    // (src/acmmp_definitions.cpp:306-379).
    void run_band(acmmp_ctx *eng, const Pass &pass, ViewState &out, hipStream_t cs) {
        const auto [lo, hi] = band_rows(out.H, g_.rank);
        BandCtx b{this, cs, {}, {}, {}};
        for (int run = 0; run < (pass.planar ? 2 : 1); ++run) {
            if (run) {
                acmmp_check(acmmp_set_plane_hypotheses_device(eng, out.planes.p, out.costs.p),
                            "acmmp_set_plane_hypotheses_device", eng);
                int nsp = 0, ntri = 0;
                acmmp_check(acmmp_prepare_planar_prior(eng, &nsp, &ntri), "acmmp_prepare_planar_prior", eng);
            }
            const int rc = acmmp_run_patchmatch_band(eng, lo, hi, &Driver::band_exchange, &b);
            if (!b.err.empty()) fail("band exchange: " + b.err);
            acmmp_check(rc, "acmmp_run_patchmatch_band", eng);
            acmmp_check(acmmp_export_results(eng, out.planes.p, out.costs.p, nullptr), "acmmp_export_results", eng);
            acmmp_check(acmmp_synchronize(eng), "acmmp_synchronize", eng);
            gather_bands(out, cs);
        }
        extract_depth(out, cs);
    }

    void write_outputs(int v, const ViewState &s, bool geom) {
        const std::string folder = result_folder(output_folder_, problems_[(size_t)v].ref_image_id);
        ::mkdir(folder.c_str(), 0777);
        const size_t P = (size_t)s.W * s.H;
        std::vector<float> pl(P * 4), co(P);
        hip_check(hipMemcpy(pl.data(), s.planes.p, pl.size() * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy");
        hip_check(hipMemcpy(co.data(), s.costs.p, co.size() * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy");
        if (write_view_maps(folder, geom, s.H, s.W, pl.data(), co.data()))
            fail("cannot write the .dmb outputs of view " + std::to_string(problems_[(size_t)v].ref_image_id));
    }

    void run_pass(const Pass &pass) {
        std::vector<Task> tasks;
        for (int v : plan_.mine(g_.rank)) tasks.push_back({v, pass});
        std::vector<ViewState> next(state_.size());
        // views off a shared queue, one host thread per engine
        std::atomic<size_t> q{0};
        std::vector<std::string> errs(engines_.size());
        auto worker = [&](size_t e) {
            try {
                hip_check(hipSetDevice(o_.device), "hipSetDevice");  // per thread: the output buffers go there
                for (size_t k; (k = q++) < tasks.size();)
                    next[(size_t)tasks[k].view] = compute(engines_[e], tasks[k], copy_[e], &Driver::run_whole);
            } catch (const std::exception &ex) {
                errs[e] = ex.what();
                q = tasks.size();
            }
        };
        {
            Clock c(this, "compute");
            std::vector<std::thread> th;
            for (size_t e = 0; e < engines_.size(); ++e) th.emplace_back(worker, e);
            for (auto &t : th) t.join();
        }
        for (auto &e : errs)
            if (!e.empty()) fail(e);
        if (!plan_.split.empty()) {  // the tail views, every rank on a band of each
            Clock c(this, "split_compute");
            for (int v : plan_.split)
                next[(size_t)v] = compute(engines_[0], Task{v, pass}, copy_[0], &Driver::run_band);
        }
        {
            Clock c(this, "flush_writes");
            flush_writes();  // the previous pass's writers still read the state replaced below
        }
        Clock c(this, "exchange");
        // state (every rank holds the split views' full state), then the padded
        // all-gather of the depth maps; the outputs are written while the
        // all-gather waits for the other ranks and the next pass computes
        for (int v : computed()) state_[(size_t)v] = std::move(next[(size_t)v]);
        for (int v : owned()) {
            const ViewState &s = state_[(size_t)v];
            depths_.put(v, s.depth.p, s.W, s.H);
        }
        if (o_.write_outputs) start_writes(pass.geom);
        depths_.gather(ex_);
        pass_index_++;
    }

    // JointBilateralUpsampling of each computed view's previous-scale depth
    // to this scale's image (src/ACMMP.cpp:964-1087) on the device, kept
    // there for the hierarchy pass
    void jbu() {
        for (int v : computed()) {
            ViewState &s = state_[(size_t)v];
            const int id = problems_[(size_t)v].ref_image_id;
            const acmmp_camera &c = cams_.at(id);
            s.jbu = DevBuf((size_t)c.width * c.height);
            int isc = 0;
            acmmp_check(acmmp_joint_bilateral_upsample_device(o_.device, images_.at(id).p, c.width, c.height,
                                                              s.depth.p, s.W, s.H, s.jbu.p, &isc),
                        "acmmp_joint_bilateral_upsample_device");
            if (isc <= 1) fail("view " + std::to_string(id) + ": JBU image scale 1 (nothing to upsample)");
        }
    }

    VpOptions o_;
    Group &g_;
    Exchange ex_;
    std::string output_folder_;
    std::vector<acmmp_problem> problems_;
    std::map<int, int> index_of_;
    int max_down_ = -1;
    Plan plan_;  // who owns, computes and splits which view; the all-gather slots
    std::vector<acmmp_ctx *> engines_;
    std::vector<hipStream_t> copy_;  // per engine: the driver's device-to-device copies
    std::map<int, DevBuf> images_;
    std::map<int, acmmp_texture *> textures_;  // ~ the reference's texture objects, per image and scale
    std::map<int, acmmp_camera> cams_;
    std::map<int, PriorMapsDev> prior_maps_;  // -p, first pass only: per problem index
    std::vector<int> height_, width_;  // of every view at this scale
    int hmax_ = 0, wmax_ = 0;
    PaddedGather gathered_images_;  // this scale's images of every view (textures borrow it)
    PaddedGather depths_;           // the previous pass's depth maps of every view
    std::vector<ViewState> state_;  // per problem index: the views this rank computes
    int pass_index_ = 0;
    std::vector<std::thread> writers_;
    std::vector<std::string> write_errs_;
    std::map<std::string, double> phase_s_;
};

int env_int(const char *name, int dflt) {
    const char *v = std::getenv(name);
    return v && *v ? std::atoi(v) : dflt;
}

}  // namespace

int run_view_parallel(const VpOptions &opt) {
    try {
        const int rank = env_int("RANK", 0), world = env_int("WORLD_SIZE", 1);
        VpOptions o = opt;
        if (o.device < 0) o.device = env_int("LOCAL_RANK", 0);
        const char *addr = std::getenv("MASTER_ADDR");
        const int port = env_int("ACMMP_RDZV_PORT", env_int("MASTER_PORT", 29500) + 1);
        if (rank < 0 || world < 1 || rank >= world) fail("bad RANK / WORLD_SIZE");
        if (o.exchange_auto && world == 1) o.exchange_rccl = false;  // nothing to exchange
        using clk = std::chrono::steady_clock;
        const auto t0 = clk::now();
        Group g(rank, world, addr && *addr ? addr : "127.0.0.1", port);
        double init_s = 0, run_s = 0;
        clk::time_point t3;
        {
            Driver d(o, g);  // problems, LPT, RCCL communicator, engines
            const auto t1 = clk::now();
            d.run();
            const auto t2 = clk::now();
            init_s = std::chrono::duration<double>(t1 - t0).count();
            run_s = std::chrono::duration<double>(t2 - t1).count();
            t3 = clk::now();
        }
        if (std::getenv("ACMMP_HOST_TIMING"))
            std::fprintf(stderr, "[rank %d] init=%.2fs run=%.2fs teardown=%.2fs\n", rank, init_s, run_s,
                         std::chrono::duration<double>(clk::now() - t3).count());
        if (rank == 0 && o.verbose)
            std::printf("view-parallel: %d ranks (%s exchange), maps under %s%s\n", world,
                        o.exchange_rccl ? "RCCL" : "TCP", o.dense.c_str(), o.output_dir.c_str());
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "acmmp_main --view_parallel: %s\n", e.what());
        return 1;
    }
}
