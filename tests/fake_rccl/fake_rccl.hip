// fake_rccl.hip -- TEST DOUBLE of librccl for the data-parallel tests (tests/test_parity_gpu.py, tests/test_dp_native_gpu.py).
// Not part of the product; built by __graft_entry__.build() into tests/fake_rccl/libfake_rccl.so and selected with L3_RCCL_LIB
// (csrc/comm.hip binds whatever library that names).  Two modes:
//
// IN-PROCESS (default).  Two ranks cannot share one GPU under the real RCCL, and at world size 1 an in-place all-reduce is an
// identity, so a collective launched BEFORE its bucket's backward finished -- or an Adam step launched before the last collective --
// would go unnoticed.  This mode makes the collective visible and slow:
//   ncclAllReduce(sum)  = "world" ranks that all hold this rank's data: out = world * in, on the caller's stream,
//                         behind a kernel that spins for FAKE_RCCL_DELAY_US (default 300) microseconds;
//   ncclAllReduce(max)  = identity;
//   ncclAllGather       = every rank's slot holds this rank's data, behind the same delay.
// FAKE_RCCL_BLOCKS / FAKE_RCCL_THREADS / FAKE_RCCL_LDS_KB give the delay kernel the CU footprint of a real ring kernel.
// With an engine whose global batch is world x its own batch (loss gradients scaled by 1 / (world * B)) the reduced
// gradients equal, bit for bit (powers of two), those of the plain single-GPU step at global batch B -- if and only if
// every bucket is reduced after its last writer and before Adam reads it.
//
// INTER-PROCESS (FAKE_RCCL_IPC_DIR=<dir>).  Real ranks in separate processes that hold different data, all on one GPU: the
// collectives really combine what the ranks hold.  ncclGetUniqueId writes a marker and a random token; ncclCommInitRank maps
// <dir>/<token>, a regular file (rank 0 creates it) holding a sense-reversing barrier and one staging slot of SLOT_BYTES per rank,
// and waits for all ranks.  Every collective runs synchronously on the host: wait for the stream (the caller's event waits queued
// on it), copy this rank's data into its slot on that stream, barrier, combine the slots in rank order 0..world-1 (a plain fp32 /
// fp64 `+` for ncclSum, max for ncclMax; ncclAllGather: slot r -> recv + r * count), barrier, copy the result back on the stream;
// buffers larger than a slot go in chunks.  No kernel is launched and no delay is added.  Every barrier gives up after
// FAKE_RCCL_IPC_TIMEOUT_S seconds (default 60) with ncclSystemError: a dead peer fails the call instead of hanging it.
// ncclCommDestroy unmaps the file; rank 0 unlinks it.
//
// Both modes: FAKE_RCCL_FAIL_AT=<n> makes the n-th collective call of the process (all-reduce or all-gather, counted from 1)
// return ncclSystemError; fake_rccl_launches() counts the collectives that ran.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

// inter-process mode: the head of the mapped file, followed by one staging slot per rank
struct IpcShared {
    char magic[16];
    int world;
    std::atomic<int> arrived;       // ranks at the current barrier
    std::atomic<int> sense;         // flipped by the last rank to arrive
};

struct FakeComm {
    int world, rank;
    long launches;
    IpcShared* shm = nullptr;       // inter-process mode: the mapped file (nullptr: in-process mode)
    size_t map_bytes = 0;
    std::string path;
    int sense = 0;                  // this rank's side of the sense-reversing barrier
};

namespace {

// One workgroup of the collective's stand-in: holds its threads' registers and `lds_bytes` of LDS for `cycles` of the 100-MHz
// wall clock, counted from the moment the workgroup itself starts (a workgroup that has to wait for a CU holds it that much later).
__global__ void spin_kernel(long long cycles, int lds_bytes, int* sink) {
    extern __shared__ int lds[];
    if (lds_bytes > 0) lds[threadIdx.x] = (int)threadIdx.x;         // the allocation is what matters; keep it live
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < cycles) __builtin_amdgcn_s_sleep(32);
    if (lds_bytes > 0 && lds[(threadIdx.x + 1) % blockDim.x] < 0) *sink = 1;
}

int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v != nullptr && *v ? atoi(v) : dflt;
}

// The delay in front of every collective.  Default: one 64-thread workgroup, no LDS (rounds 3-5: visible and slow, but with no
// footprint).  A real RCCL ring kernel is tens of 256-512-thread workgroups with LDS and many registers that cannot share a CU
// with a 160-KiB-LDS convolution workgroup: FAKE_RCCL_BLOCKS x FAKE_RCCL_THREADS threads x FAKE_RCCL_LDS_KB KiB of LDS, each
// workgroup holding its CU share for FAKE_RCCL_DELAY_US.
void fake_delay(hipStream_t stream) {
    const long long us = env_int("FAKE_RCCL_DELAY_US", 300);
    if (us <= 0) return;
    const int blocks = env_int("FAKE_RCCL_BLOCKS", 1), threads = env_int("FAKE_RCCL_THREADS", 64), lds = env_int("FAKE_RCCL_LDS_KB", 0) * 1024;
    static int* sink = nullptr;
    if (sink == nullptr && hipMalloc((void**)&sink, 64) != hipSuccess) return;
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)spin_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipLaunchKernelGGL(spin_kernel, dim3(blocks < 1 ? 1 : blocks), dim3(threads < 64 ? 64 : threads > 1024 ? 1024 : threads), (size_t)lds, stream,
                       us * 100, lds, sink);      // wall_clock64: 100 MHz
}

template <typename T>
__global__ void scale_kernel(const T* in, T* out, size_t n, T f) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[i] * f;
}

// ncclMax with a peer that holds `peer` in element `at` (FAKE_RCCL_MAX_PEER="<index>:<value>"): a rank that was configured differently
__global__ void max_peer_kernel(const double* in, double* out, size_t n, int at, double peer) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (int)i == at && peer > in[i] ? peer : in[i];
}

long g_total_launches = 0;

// FAKE_RCCL_FAIL_AT=<n>: the n-th collective call of the process fails (both modes)
bool injected_failure() {
    static long calls = 0;
    return ++calls == env_int("FAKE_RCCL_FAIL_AT", 0);
}

// ---- inter-process mode (FAKE_RCCL_IPC_DIR) ----------------------------------------------------------------------------------
constexpr char kIpcMarker[] = "fake-rccl-ipc";
constexpr size_t kTokenAt = 16, kTokenLen = 32;     // the token's hex digits in ncclUniqueId::internal
constexpr size_t HEADER_BYTES = 4096, SLOT_BYTES = size_t(1) << 20;

static_assert(sizeof(IpcShared) <= HEADER_BYTES, "header");
static_assert(std::atomic<int>::is_always_lock_free, "the barrier's counters are shared between processes");

const char* ipc_dir() {
    const char* d = getenv("FAKE_RCCL_IPC_DIR");
    return d != nullptr && *d ? d : nullptr;
}

std::chrono::steady_clock::time_point ipc_deadline() {
    return std::chrono::steady_clock::now() + std::chrono::seconds(env_int("FAKE_RCCL_IPC_TIMEOUT_S", 60));
}

unsigned char* ipc_slot(const FakeComm* c, int r) {
    return reinterpret_cast<unsigned char*>(c->shm) + HEADER_BYTES + (size_t)r * SLOT_BYTES;
}

// sense-reversing barrier of the ranks that share the file; false once FAKE_RCCL_IPC_TIMEOUT_S has passed
bool ipc_barrier(FakeComm* c) {
    IpcShared* s = c->shm;
    c->sense ^= 1;
    if (s->arrived.fetch_add(1) == c->world - 1) {
        s->arrived.store(0);
        s->sense.store(c->sense);
        return true;
    }
    const auto deadline = ipc_deadline();
    while (s->sense.load() != c->sense) {
        if (std::chrono::steady_clock::now() > deadline) return false;
        std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
    return true;
}

void ipc_release(FakeComm* c) {
    if (c->shm != nullptr) munmap(c->shm, c->map_bytes);
    c->shm = nullptr;
    if (c->rank == 0 && !c->path.empty()) unlink(c->path.c_str());
    c->path.clear();
}

// rank 0 creates <dir>/<token> complete (a temporary name, then rename), the others wait for it to appear; then all ranks meet
ncclResult_t ipc_init(FakeComm* c, const ncclUniqueId& id) {
    if (memcmp(id.internal, kIpcMarker, sizeof(kIpcMarker)) != 0) return ncclInvalidArgument;     // not an id of this mode
    c->path = std::string(ipc_dir()) + "/" + std::string(id.internal + kTokenAt, kTokenLen);
    c->map_bytes = HEADER_BYTES + (size_t)c->world * SLOT_BYTES;
    int fd = -1;
    void* p = MAP_FAILED;
    if (c->rank == 0) {
        const std::string tmp = c->path + ".tmp" + std::to_string((long)getpid());
        fd = open(tmp.c_str(), O_RDWR | O_CREAT | O_EXCL, 0600);
        if (fd < 0) return ncclSystemError;
        if (ftruncate(fd, (off_t)c->map_bytes) == 0) p = mmap(nullptr, c->map_bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
        close(fd);
        if (p != MAP_FAILED) {
            IpcShared* s = static_cast<IpcShared*>(p);
            memcpy(s->magic, kIpcMarker, sizeof(kIpcMarker));
            s->world = c->world;
            s->arrived.store(0);
            s->sense.store(0);
        }
        if (p == MAP_FAILED || rename(tmp.c_str(), c->path.c_str()) != 0) {
            if (p != MAP_FAILED) munmap(p, c->map_bytes);
            unlink(tmp.c_str());
            c->path.clear();
            return ncclSystemError;
        }
    } else {
        const auto deadline = ipc_deadline();
        while ((fd = open(c->path.c_str(), O_RDWR)) < 0) {
            if (errno != ENOENT || std::chrono::steady_clock::now() > deadline) {
                c->path.clear();
                return ncclSystemError;
            }
            std::this_thread::sleep_for(std::chrono::milliseconds(1));
        }
        struct stat st;
        if (fstat(fd, &st) == 0 && (size_t)st.st_size == c->map_bytes)
            p = mmap(nullptr, c->map_bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
        close(fd);
        c->path.clear();            // rank 0 owns the name
        if (p == MAP_FAILED) return ncclInvalidArgument;       // another world size than rank 0's
    }
    c->shm = static_cast<IpcShared*>(p);
    if (memcmp(c->shm->magic, kIpcMarker, sizeof(kIpcMarker)) != 0 || c->shm->world != c->world) {
        ipc_release(c);
        return ncclInvalidArgument;
    }
    if (!ipc_barrier(c)) {          // every rank has mapped the file
        ipc_release(c);
        return ncclSystemError;
    }
    return ncclSuccess;
}

// `bytes` of this rank's data into its slot, on `stream`
ncclResult_t ipc_stage(FakeComm* c, const void* src, size_t bytes, hipStream_t stream) {
    if (hipMemcpyAsync(ipc_slot(c, c->rank), src, bytes, hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)
        return ncclUnhandledCudaError;
    return ncclSuccess;
}

template <typename T>
ncclResult_t ipc_allreduce(FakeComm* c, const T* send, T* recv, size_t count, bool is_max, hipStream_t stream) {
    const size_t per = SLOT_BYTES / sizeof(T);
    std::vector<T> acc(count < per ? count : per);
    if (hipStreamSynchronize(stream) != hipSuccess) return ncclUnhandledCudaError;     // the caller's event waits on `stream`
    for (size_t off = 0; off < count; off += per) {
        const size_t m = count - off < per ? count - off : per;
        ncclResult_t r = ipc_stage(c, send + off, m * sizeof(T), stream);
        if (r != ncclSuccess) return r;
        if (!ipc_barrier(c)) return ncclSystemError;
        memcpy(acc.data(), ipc_slot(c, 0), m * sizeof(T));
        for (int q = 1; q < c->world; ++q) {            // rank order, one plain operation per element and rank
            const T* s = reinterpret_cast<const T*>(ipc_slot(c, q));
            for (size_t i = 0; i < m; ++i) acc[i] = is_max ? (s[i] > acc[i] ? s[i] : acc[i]) : acc[i] + s[i];
        }
        if (!ipc_barrier(c)) return ncclSystemError;    // nobody refills a slot before every rank has read it
        if (hipMemcpyAsync(recv + off, acc.data(), m * sizeof(T), hipMemcpyHostToDevice, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess)
            return ncclUnhandledCudaError;
    }
    return ncclSuccess;
}

ncclResult_t ipc_allgather(FakeComm* c, const float* send, float* recv, size_t count, hipStream_t stream) {
    const size_t per = SLOT_BYTES / sizeof(float);
    if (hipStreamSynchronize(stream) != hipSuccess) return ncclUnhandledCudaError;
    for (size_t off = 0; off < count; off += per) {
        const size_t m = count - off < per ? count - off : per;
        ncclResult_t r = ipc_stage(c, send + off, m * sizeof(float), stream);
        if (r != ncclSuccess) return r;
        if (!ipc_barrier(c)) return ncclSystemError;
        for (int q = 0; q < c->world; ++q)
            if (hipMemcpyAsync(recv + (size_t)q * count + off, ipc_slot(c, q), m * sizeof(float), hipMemcpyHostToDevice, stream) != hipSuccess)
                return ncclUnhandledCudaError;
        if (hipStreamSynchronize(stream) != hipSuccess) return ncclUnhandledCudaError;
        if (!ipc_barrier(c)) return ncclSystemError;
    }
    return ncclSuccess;
}

}  // namespace

extern "C" {

ncclResult_t ncclGetVersion(int* version) {
    *version = 99999;
    return ncclSuccess;
}

ncclResult_t ncclGetUniqueId(ncclUniqueId* id) {
    memset(id, 0, sizeof(*id));
    if (ipc_dir() == nullptr) {
        memcpy(id->internal, "fake-rccl", 9);
        return ncclSuccess;
    }
    unsigned char b[kTokenLen / 2];
    FILE* f = fopen("/dev/urandom", "rb");
    const bool got = f != nullptr && fread(b, 1, sizeof(b), f) == sizeof(b);
    if (f != nullptr) fclose(f);
    if (!got) return ncclSystemError;
    memcpy(id->internal, kIpcMarker, sizeof(kIpcMarker));
    static const char hex[] = "0123456789abcdef";
    for (size_t i = 0; i < sizeof(b); ++i) {
        id->internal[kTokenAt + 2 * i] = hex[b[i] >> 4];
        id->internal[kTokenAt + 2 * i + 1] = hex[b[i] & 15];
    }
    return ncclSuccess;
}

ncclResult_t ncclCommInitRank(ncclComm_t* comm, int nranks, ncclUniqueId id, int rank) {
    if (nranks < 1 || rank < 0 || rank >= nranks) return ncclInvalidArgument;
    FakeComm* c = new FakeComm();
    c->world = nranks;
    c->rank = rank;
    if (ipc_dir() != nullptr) {
        const ncclResult_t r = ipc_init(c, id);
        if (r != ncclSuccess) {
            delete c;
            return r;
        }
    }
    *comm = reinterpret_cast<ncclComm_t>(c);
    return ncclSuccess;
}

ncclResult_t ncclCommDestroy(ncclComm_t comm) {
    FakeComm* c = reinterpret_cast<FakeComm*>(comm);
    ipc_release(c);
    delete c;
    return ncclSuccess;
}

const char* ncclGetErrorString(ncclResult_t r) {
    if (r == ncclSuccess) return "no error";
    if (r == ncclSystemError) return "fake rccl: system error (FAKE_RCCL_FAIL_AT, or a peer that did not arrive in time)";
    return "fake rccl error";
}

ncclResult_t ncclAllReduce(const void* send, void* recv, size_t count, ncclDataType_t dt, ncclRedOp_t op, ncclComm_t comm,
                           hipStream_t stream) {
    FakeComm* c = reinterpret_cast<FakeComm*>(comm);
    if (injected_failure()) return ncclSystemError;
    if (c->shm != nullptr) {
        ncclResult_t r = dt == ncclFloat    ? ipc_allreduce(c, (const float*)send, (float*)recv, count, op == ncclMax, stream)
                         : dt == ncclDouble ? ipc_allreduce(c, (const double*)send, (double*)recv, count, op == ncclMax, stream)
                                            : ncclInvalidArgument;
        if (r == ncclSuccess) {
            ++c->launches;
            ++g_total_launches;
        }
        return r;
    }
    fake_delay(stream);
    const float f = op == ncclSum ? (float)c->world : 1.f;
    const unsigned blocks = (unsigned)((count + 255) / 256);
    if (const char* mp = getenv("FAKE_RCCL_MAX_PEER"); mp != nullptr && op == ncclMax && dt == ncclDouble) {
        const char* colon = strchr(mp, ':');
        hipLaunchKernelGGL(max_peer_kernel, dim3(blocks), dim3(256), 0, stream, (const double*)send, (double*)recv, count, atoi(mp),
                           colon ? atof(colon + 1) : 0.0);
        ++c->launches;
        ++g_total_launches;
        return ncclSuccess;
    }
    if (dt == ncclFloat)
        hipLaunchKernelGGL(scale_kernel<float>, dim3(blocks), dim3(256), 0, stream, (const float*)send, (float*)recv, count, f);
    else if (dt == ncclDouble)
        hipLaunchKernelGGL(scale_kernel<double>, dim3(blocks), dim3(256), 0, stream, (const double*)send, (double*)recv, count,
                           (double)f);
    else
        return ncclInvalidArgument;
    ++c->launches;
    ++g_total_launches;
    return ncclSuccess;
}

// in-process mode: "world" ranks that all hold this rank's data: every slot of recv = send (behind the same delay as an all-reduce)
ncclResult_t ncclAllGather(const void* send, void* recv, size_t count, ncclDataType_t dt, ncclComm_t comm, hipStream_t stream) {
    FakeComm* c = reinterpret_cast<FakeComm*>(comm);
    if (injected_failure()) return ncclSystemError;
    if (dt != ncclFloat) return ncclInvalidArgument;
    if (c->shm != nullptr) {
        ncclResult_t r = ipc_allgather(c, (const float*)send, (float*)recv, count, stream);
        if (r == ncclSuccess) {
            ++c->launches;
            ++g_total_launches;
        }
        return r;
    }
    fake_delay(stream);
    for (int r = 0; r < c->world; ++r)
        if (hipMemcpyAsync((float*)recv + (size_t)r * count, send, count * sizeof(float), hipMemcpyDeviceToDevice, stream) != hipSuccess)
            return ncclUnhandledCudaError;
    ++c->launches;
    ++g_total_launches;
    return ncclSuccess;
}

// test hook: collectives launched so far in this process
long fake_rccl_launches() { return g_total_launches; }

}  // extern "C"
