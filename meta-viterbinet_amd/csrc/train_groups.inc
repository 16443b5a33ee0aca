// train_groups.inc -- the training kernels spread over several workgroups (one per 32-sample chunk), included by
// mvn_hip.hip after maml_train.inc.
//
// online_train.inc / maml_train.inc run a whole training call on ONE workgroup: right for the 32-sample minibatch of
// select_batch (one chunk per iteration, nothing to share), wasteful for the full-word iterations of
// metavnet_trainer.py:41-64 and for the meta-learning step of trainer.py:425-453, whose 5 + 5 + 9 chunks per step are
// independent given the weights.  Here every chunk of a pass has its own workgroup on its own CU:
//   * each workgroup keeps a full copy of the parameters (and, online kernel, both Adam moments) in LDS and updates it
//     identically, so weights never travel;
//   * after its chunk a workgroup writes its gradient vector (24 KB) to a slot of the caller's workspace; ONE device-wide
//     barrier later every workgroup adds all slots IN CHUNK ORDER -- exactly the sums the single-workgroup kernels
//     build by accumulating chunk after chunk ((0 + c0) + c1) + ..., so results are bit-identical to them (tests/);
//   * slots are double-buffered by step parity: one barrier per exchange is enough.
// The barrier is a monotone arrival counter in the workspace (zeroed by the launcher), spun on with s_sleep by one
// thread per workgroup.  Everything one workgroup writes for another (gradient slots, the chunk losses) is stored
// WRITE-THROUGH (sc1) and read by sc1 loads that bypass the reader's L1 (cdna_hip_programming.md, Guideline 16, form R1 with
// the counter in place of the flag; MI355X_MICROARCH.md "Valid forms", first row of the table): every storing wave drains
// its stores (s_waitcnt vmcnt(0)), the workgroup's barrier, ONE lane's relaxed agent-scope add, a relaxed sc1 poll, the
// workgroup's barrier again, sc1 loads.  That form needs neither the L2 write-back of an agent-scope release (1.7-6.5 us with
// 24 KB freshly written per workgroup) nor the L1 invalidate of an acquire (1.7 us) -- per exchange, on every workgroup;
// MVN_XCHG_SC1=0 at compile time keeps the release / acquire form with plain stores and loads (A/B).
// ONE XCD PER TRIAL (group_place, set_same_xcd below): the launcher's grid puts a trial's workgroups on one XCD where the
// dispatcher deals blocks round-robin (observed, not promised); the workgroups establish it themselves from HW_REG_XCC_ID
// across the launch's first device-wide barrier, and a trial that finds itself on one XCD keeps the exchange in that XCD's L2:
// plain stores (their lines stay in the L2), one arrival tag per workgroup there instead of the device-wide counter, and the
// same sc1 loads (L1 bypassed, served by the L2).  A trial that did not land on one XCD runs the write-through form above.
// The launch is an ordinary one with at most kTrainMaxGroups
// 1024-thread workgroups per trial and never more workgroups than the device has CUs (the launcher splits the trials of a
// call over several launches if need be), so all of them are resident at once; the spin is bounded all the same, so that a
// launch that somehow cannot become resident ends -- GroupSync::failed set, the trial's status word set to 1, NaN in the
// weights -- instead of hanging the device.  Trials (gridDim.y, mvn_vnet_*_train_trials_f32) never share a GroupSync: each
// has its own region of the workspace (counter, slots, private moment copies), `ws_stride` floats apart.
constexpr int kTrainMaxGroups = 32;
constexpr unsigned kGroupSpinLimit = 1u << 22;  // x ~0.25 us per poll (s_sleep 8 + the load): about a second
#ifdef MVN_TEST_HOOKS  // the tests' build only (libmvn_hip_hooks.so): mvn_test_hooks() lowers the limit / adds phantom arrivals
std::atomic<unsigned> g_group_spin_limit{kGroupSpinLimit};  // host copy handed to every launch
std::atomic<int> g_group_phantoms{0};                       // the barriers wait for this many workgroups that do not exist
inline unsigned group_spin_limit() { return g_group_spin_limit.load(std::memory_order_relaxed); }
inline int group_phantoms() { return g_group_phantoms.load(std::memory_order_relaxed); }
#else
inline unsigned group_spin_limit() { return kGroupSpinLimit; }
inline int group_phantoms() { return 0; }
#endif

#ifndef MVN_XCHG_SC1
#define MVN_XCHG_SC1 1
#endif
struct GroupSync {  // head of a trial's workspace region: three 128-byte lines of their own
    unsigned arrived, failed, xcc_mask, pad[29];  // xcc_mask: bit x set by every workgroup of the trial that runs on XCD x
    unsigned tags[32];                            // one XCD per trial: workgroup w's arrival = the number of the exchange, stored here
    unsigned placement, pad2[31];                 // what the trial's workgroups found (1 = one XCD, L2 exchange; 2 = several, write-through)
};
static_assert(sizeof(GroupSync) == 384, "three lines");

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
// A trial's workspace region as a buffer resource: float offsets from its base, 16-byte and 4-byte accesses with the sc1
// bit (aux 16) or plain, by MVN_XCHG_SC1
struct SlotIO {
    __amdgpu_buffer_rsrc_t rs;
    float *base;
    // same_xcd (workgroup-uniform, the same in every workgroup of the trial; set_same_xcd()): all workgroups of the trial share
    // ONE L2.  Their stores may then stay plain: a plain store's line is kept in that L2 (MI355X_MICROARCH.md, "stores of each
    // flavour"), where the readers' sc1 loads -- which bypass their L1 and are served by the L2 -- find it, instead of travelling
    // to memory and back at the cross-XCD rate.  The arrival goes the same way (groups_barrier, `local`); everything else of the
    // exchange is unchanged (each storing wave's s_waitcnt vmcnt(0), the workgroup barriers, sc1 polls and sc1 loads only).
    bool same_xcd = false;
    __device__ SlotIO(float *b, unsigned bytes) : rs(__builtin_amdgcn_make_buffer_rsrc(b, 0, bytes, 0x00020000)), base(b) {}
    __device__ __forceinline__ void store4(size_t f, const float4 v) const {
#if MVN_XCHG_SC1
        const u32x4 u = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
        if (same_xcd) __builtin_amdgcn_raw_buffer_store_b128(u, rs, (int)(f * 4), 0, 0);
        else __builtin_amdgcn_raw_buffer_store_b128(u, rs, (int)(f * 4), 0, 16);
#else
        *reinterpret_cast<float4 *>(base + f) = v;
#endif
    }
    __device__ __forceinline__ float4 load4(size_t f) const {
#if MVN_XCHG_SC1
        const u32x4 u = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(f * 4), 0, 16);
        return make_float4(__uint_as_float(u[0]), __uint_as_float(u[1]), __uint_as_float(u[2]), __uint_as_float(u[3]));
#else
        return *reinterpret_cast<const float4 *>(base + f);
#endif
    }
    __device__ __forceinline__ void store1(size_t f, float v) const {
#if MVN_XCHG_SC1
        if (same_xcd) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rs, (int)(f * 4), 0, 0);
        else __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rs, (int)(f * 4), 0, 16);
#else
        base[f] = v;
#endif
    }
    __device__ __forceinline__ float load1(size_t f) const {
#if MVN_XCHG_SC1
        return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (int)(f * 4), 0, 16));
#else
        return base[f];
#endif
    }
};

// a slot: the gradient vector, the chunk's loss, padding to whole 128-byte lines (no line is shared by two workgroups' stores)
__host__ __device__ inline size_t train_group_slot_floats(int S) { return ((size_t)train_layout(S).P4 + 4 + 31) & ~(size_t)31; }
inline size_t train_groups_workspace_bytes(int S, int groups) {
    return sizeof(GroupSync) + (size_t)2 * groups * train_group_slot_floats(S) * sizeof(float);
}

// every workgroup of the launch has called this `epoch` times when it returns (false: the wait was abandoned).
// local (workgroup-uniform, the same in all workgroups of the trial: SlotIO::same_xcd): the trial's workgroups share one L2 and
// the barrier stays there too: workgroup w (of n_groups, none of them phantoms) stores the exchange's number -- epoch minus
// `local_base`, the epochs that went through the device-wide counter before -- into tags[w] with a plain store (its line stays
// in the XCD's L2) after all its waves' payload stores have been acknowledged, and the first n_groups lanes of wave 0 poll
// one tag each with sc1 loads (L1 bypassed, served by that L2) until every tag has reached the number: the payload of every
// workgroup is then in the L2, and every workgroup has finished reading the previous exchanges (it arrives after them).
__device__ __forceinline__ bool groups_barrier(GroupSync *gs, unsigned n_groups, unsigned &epoch, unsigned spin_limit, bool local = false,
                                               unsigned local_base = 0, int w = 0, bool skip_tag = false) {
    __shared__ int ok;
    ++epoch;
#if MVN_XCHG_SC1
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // EVERY storing wave: its stores have left the CU (write-through: for memory; plain: for the L2)
#endif
    __syncthreads();
#if MVN_XCHG_SC1
    if (local) {
        if (threadIdx.x < 64) {
            const unsigned number = epoch - local_base;
            // Hardware assumption (MI355X_MICROARCH.md, "stores of each scope"): the vector L1 is write-through, so this plain
            // (workgroup-scope) store's line reaches the XCD's L2 and STAYS there, where the pollers' agent-scope (sc1) loads of the
            // same XCD find it.  Formally the scopes do not match; an agent-scope store would add the sc1 bit = write the line
            // through to memory, which is exactly the traffic the one-XCD form exists to avoid.  A trial whose workgroups are not
            // on one XCD never takes this branch (set_same_xcd).
            // (skip_tag: the tests' hook -- this workgroup "forgets" to publish, the others must give up and say so)
            if (threadIdx.x == 0 && !skip_tag) __hip_atomic_store(&gs->tags[w], number, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            unsigned spins = 0;
            bool good = true;
            for (;;) {
                const unsigned v = threadIdx.x < n_groups ? __hip_atomic_load(&gs->tags[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : number;
                if (__all((int)(v - number) >= 0)) break;
                __builtin_amdgcn_s_sleep(1);
                if (++spins > spin_limit || __hip_atomic_load(&gs->failed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                    __hip_atomic_store(&gs->failed, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    good = false;
                    break;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // (no instruction: keeps the compiler from moving loads above the poll)
            if (threadIdx.x == 0) ok = good;
        }
        __syncthreads();
        return ok != 0;
    }
#endif
    if (threadIdx.x == 0) {
#if !MVN_XCHG_SC1
        // ONE release (L2 write-back) before the arrival and ONE acquire (invalidate) after the wait; the counter itself is
        // polled with relaxed loads (an acquire load would invalidate the caches at every poll).  The explicit waits keep the
        // arrival behind the write-back and the barrier behind the invalidate (MI355X_MICROARCH.md, "Compiler hazard": the
        // compiler may drop the s_waitcnt that belongs to buffer_wbl2 when it can prove its own counter empty).
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
        __hip_atomic_fetch_add(&gs->arrived, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unsigned spins = 0;
        bool good = true;
        while (__hip_atomic_load(&gs->arrived, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < epoch * n_groups) {
            __builtin_amdgcn_s_sleep(8);
            if (++spins > spin_limit || __hip_atomic_load(&gs->failed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                __hip_atomic_store(&gs->failed, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                good = false;
                break;
            }
        }
#if MVN_XCHG_SC1
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // (no instruction: keeps the compiler from moving loads above the poll)
#else
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // drop this CU's stale lines before anyone reads the other slots
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // (the invalidate completes asynchronously: wait for it)
#endif
        ok = good;
    }
    __syncthreads();
    return ok != 0;
}

// workgroup-uniform: has any workgroup of the trial abandoned a wait?  (one relaxed agent-scope load per thread of a word that
// sits in L2; called once, when a trial ends)
__device__ __forceinline__ bool trial_failed(GroupSync *gs) {
    return __hip_atomic_load(&gs->failed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
}

// Sum of the n_groups slots, in slot order, for the (at most two) float4s a thread owns: e4 = tid and tid + 1024
// (n4 = P4 / 4 <= 2048).  Both elements' loads of a slot are issued together and the slot loop is unrolled, so that the
// read latency of the exchange is paid a few times, not once per slot and element.  own >= 0: slot `own` is this workgroup's
// own vector, still in LDS at `mine` -- the same bits it stored, taken from there (a fifth of the exchange's read volume at 5
// workgroups per trial).
__device__ __forceinline__ void sum_slots(const SlotIO &io, size_t slots, size_t slot_floats, int n_groups, int tid, int n4, float4 (&acc)[2],
                                          int own = -1, const float *mine = nullptr) {
    const bool in1 = tid + kTrainThreads < n4;  // tid < n4 always (n4 >= 1024 for every S)
    const size_t e0 = slots + 4 * (size_t)tid, e1 = e0 + 4 * kTrainThreads;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    auto slot = [&](int c, float4 &a, float4 &b) {
        if (c == own) {
            a = reinterpret_cast<const float4 *>(mine)[tid];
            b = in1 ? reinterpret_cast<const float4 *>(mine)[tid + kTrainThreads] : zero;
        } else {
            a = io.load4(e0 + c * slot_floats);
            b = in1 ? io.load4(e1 + c * slot_floats) : zero;
        }
    };
    slot(0, acc[0], acc[1]);
#pragma unroll 4
    for (int c = 1; c < n_groups; ++c) {
        float4 a, b;
        slot(c, a, b);
        acc[0] = make_float4(acc[0].x + a.x, acc[0].y + a.y, acc[0].z + a.z, acc[0].w + a.w);
        acc[1] = make_float4(acc[1].x + b.x, acc[1].y + b.y, acc[1].z + b.z, acc[1].w + b.w);
    }
}

// What a launch of the group kernels has in common (by value): the workspace and how its barriers behave
struct GroupLaunch {
    float *workspace;      // trial r's region starts at workspace + r * ws_stride
    long long ws_stride;   // floats
    unsigned ws_bytes;     // bytes of one trial's region
    unsigned spin_limit;
    int phantoms;          // test hook (0 in production): > 0 extra arrivals every barrier waits for; -(k + 1): workgroup k of a
                           // trial skips the tag stores of the one-XCD barrier (the others must abandon the wait)
    int groups;            // > 0: the XCD-aware 1-D grid below with this many workgroups per trial; 0: grid (groups, trials)
    int trials;            // trials of this launch (XCD-aware grid: slots beyond it leave at once)
    int xcd_first;         // XCD-aware grid: slot (= XCD) of a unit its first trial takes; 0 for the trial-batched calls, rotated
                           // from launch to launch for the single-trial calls (launches in flight on several streams spread over
                           // the XCDs instead of all landing on the dispatch's first one)
};

// Which chunk of which trial a workgroup is.  Classic grid: (blockIdx.x, blockIdx.y).  XCD-aware grid (gl.groups > 0): blocks are
// dealt round-robin over the 8 XCDs (blocks b and b + 8 share one: MI355X_MICROARCH.md, "Workgroup dispatch"; observed, not
// promised), so a 1-D grid in units of 8 G blocks gives block 8 c + j of a unit to chunk c of the unit's j-th trial: the G
// workgroups of a trial then sit on ONE XCD and exchange their gradients through its L2.  Nothing depends on it for correctness:
// the workgroups establish where they run from HW_REG_XCC_ID (set_same_xcd) and keep the write-through exchange otherwise.
struct GroupPlace {
    int w, G, trial;
    bool active;
};
__device__ __forceinline__ GroupPlace group_place(const GroupLaunch &gl) {
    GroupPlace pl;
    if (gl.groups > 0) {
        const int per = 8 * gl.groups, unit = (int)blockIdx.x / per, rem = (int)blockIdx.x % per;
        pl.w = rem >> 3;
        pl.G = gl.groups;
        pl.trial = 8 * unit + (((rem & 7) - gl.xcd_first) & 7);
        pl.active = pl.trial < gl.trials;
    } else {
        pl.w = (int)blockIdx.x;
        pl.G = (int)gridDim.x;
        pl.trial = (int)blockIdx.y;
        pl.active = true;
    }
    return pl;
}
// before a trial's FIRST barrier: one lane records the XCD this workgroup runs on (and waits for the atomic to have completed)
__device__ __forceinline__ void announce_xcd(GroupSync *gs) {
    if (threadIdx.x == 0) {
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcc));
        __hip_atomic_fetch_or(&gs->xcc_mask, 1u << (xcc & 15u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the arrival (groups_barrier) comes after it
    }
}
// after that barrier: every workgroup of the trial reads the same mask (all of them have announced themselves); exactly one
// bit = one XCD.  Phantom arrivals (test hook) and a failed barrier keep the write-through exchange.
__device__ __forceinline__ void set_same_xcd(SlotIO &io, GroupSync *gs, bool good, bool allow) {
    __shared__ int same;
    if (threadIdx.x == 0) {
        const unsigned m = __hip_atomic_load(&gs->xcc_mask, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        same = good && allow && __builtin_popcount(m) == 1;
        gs->placement = same ? 1u : 2u;  // (every workgroup of the trial stores the same value; read by the tests)
    }
    __syncthreads();
    io.same_xcd = same != 0;
}
// Workgroup 0 of a trial after its last step, parameters in `p`.  ANY workgroup of the trial may have given up a wait (it then read
// incomplete slots while this one passed its barriers late but complete): the trial's failed flag decides, not only this workgroup's
// own waits.  A barrier was abandoned: make it impossible to miss (NaN weights) and tell the caller (status word).
// (A text: as a function it changes every chunked kernel.)
#define MVN_FINISH_GROUP_TRIAL(p)                                                              \
    do {                                                                                       \
        good = good && !trial_failed(gs);                                                      \
        if (!good) {                                                                           \
            for (int e = tid; e < L.P4; e += kTrainThreads) p[e] = __int_as_float(0x7fc00000); \
            if (tid == 0 && d.status) *d.status = 1;                                           \
        }                                                                                      \
        __syncthreads();                                                                       \
        store_trial_params(p, L, S, d);                                                        \
    } while (0)

// online_train_kernel's full-word mode (batch_idx == NULL), gridDim.x = ceil(T / 32) workgroups, workgroup w = chunk w,
// gridDim.y = trials (MANY) or 1
template <int SC, bool MANY>
__global__ __launch_bounds__(kTrainThreads) void online_train_groups_kernel(
    const mvn_train_trial_t one, const mvn_train_trial_t *__restrict__ many, int T, float lr, float beta1, float beta2,
    float eps, int S_rt, int lds_floats, const GroupLaunch gl) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const GroupPlace pl = group_place(gl);
    if (!pl.active) return;
    const mvn_train_trial_t &d = MANY ? many[pl.trial] : one;
    const int n_iter = d.n;
    if (n_iter <= 0) return;  // the whole trial: all its workgroups leave before any barrier
    const float *__restrict__ y = d.y;
    const int *__restrict__ labels = d.labels;
    float *__restrict__ adam_m = d.adam_m, *__restrict__ adam_v = d.adam_v, *__restrict__ loss_out = d.loss_out;
    double b1pow = d.b1pow, b2pow = d.b2pow;
    const int S = SC ? SC : S_rt;
    const TrainLayout L = train_layout(S);
    float *p = smem, *g = p + L.P4, *am = g + L.P4, *av = am + L.P4;
    const ChunkArena<kTrainChunk> A(av + L.P4);
    const int tid = threadIdx.x, w = pl.w, G = pl.G;
    float *workspace = gl.workspace + (MANY ? (long long)pl.trial * gl.ws_stride : 0);
    GroupSync *gs = reinterpret_cast<GroupSync *>(workspace);
    SlotIO io(workspace, gl.ws_bytes);
    const size_t slots = sizeof(GroupSync) / sizeof(float);  // float offset of the slots in the trial's region
    const size_t X = train_group_slot_floats(S);
    const unsigned n_arrive = (unsigned)(G + (gl.phantoms > 0 ? gl.phantoms : 0));
    const bool skip_tag = gl.phantoms < 0 && w == -gl.phantoms - 1;  // test hook: this workgroup never publishes its tag

    announce_xcd(gs);
    MVN_CLEAR_LDS_LOAD_PARAMS(kTrainThreads, p);
    moments_to_lds(am, av, adam_m, adam_v, L.Pflat, tid);
    const int c0 = w * kTrainChunk;
    const int nc = T - c0 < kTrainChunk ? T - c0 : kTrainChunk;
    if (tid < kTrainChunk) {  // the chunk is the same in every iteration
        const bool valid = tid < nc;
        A.ys[tid] = valid ? y[c0 + tid] : 0.0f;
        A.lab[tid] = valid ? labels[c0 + tid] : 0;
    }
    __syncthreads();
    const float inv_n = 1.0f / (float)T;
    unsigned epoch = 0;
    bool good = true;
    if (gl.groups > 0) {  // where do the trial's workgroups run?  (one barrier per launch; the classic grid spreads them over the XCDs)
        good = groups_barrier(gs, n_arrive, epoch, gl.spin_limit);
        set_same_xcd(io, gs, good, gl.phantoms <= 0);
    }
    for (int it = 0; it < n_iter && good; ++it) {
        if (tid == kTrainThreads - 1) A.red[kTrainChunk] = 0.0f;
        // (every workgroup keeps its own, identical, running powers)
        auto bias_corrections = [&]() { next_bias_corrections<false>(b1pow, b2pow, lr, beta1, beta2, A.red[kTrainChunk + 1], A.red[kTrainChunk + 2]); };
        // (the word's tail runs the 16-row chunk exactly where online_train_kernel does: chunk 0 is always the full form.  Every
        // workgroup WRITES its own gradient vector; the slots are then summed in chunk order, online_train_kernel's order)
        if (w > 0 && nc <= 16) grad_chunk<16, true>(p, g, L, A, nc, inv_n, S, bias_corrections);
        else grad_chunk<kTrainChunk, true>(p, g, L, A, nc, inv_n, S, bias_corrections);
        const size_t mine = slots + ((size_t)(it & 1) * G + w) * X;
        for (int e4 = tid; e4 < L.P4 / 4; e4 += kTrainThreads) io.store4(mine + 4 * (size_t)e4, reinterpret_cast<const float4 *>(g)[e4]);
        if (tid == 0) io.store1(mine + L.P4, A.red[kTrainChunk]);  // the chunk's summed loss
        good = groups_barrier(gs, n_arrive, epoch, gl.spin_limit, io.same_xcd, 1, w, skip_tag) && good;  // (every workgroup arrives; a failure is sticky)
        const size_t all = slots + (size_t)(it & 1) * G * X;
        const float step_size = A.red[kTrainChunk + 1], inv_sqrt_bc2 = A.red[kTrainChunk + 2];
        float4 tot[2];
        sum_slots(io, all, X, G, tid, L.P4 / 4, tot, w, g);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int e4 = tid + j * kTrainThreads;
            if (e4 >= L.P4 / 4) break;
            float4 p4 = reinterpret_cast<float4 *>(p)[e4], m4 = reinterpret_cast<float4 *>(am)[e4];
            float4 v4 = reinterpret_cast<float4 *>(av)[e4];
            adam4(p4, m4, v4, tot[j], beta1, beta2, eps, step_size, inv_sqrt_bc2);
            reinterpret_cast<float4 *>(am)[e4] = m4;
            reinterpret_cast<float4 *>(av)[e4] = v4;
            reinterpret_cast<float4 *>(p)[e4] = p4;
        }
        if (w == 0 && tid == 0 && loss_out) {
            float loss = io.load1(all + L.P4);
            for (int c = 1; c < G; ++c) loss += io.load1(all + c * X + L.P4);
            loss_out[it] = loss * inv_n;
        }
        __syncthreads();
    }
    if (w != 0) return;
    MVN_FINISH_GROUP_TRIAL(p);
    moments_from_lds(am, av, adam_m, adam_v, L.Pflat, tid);
}

// maml_train_kernel with one workgroup per chunk of a pass: gridDim.x = the largest chunk count of the three passes
// (support gradient, query gradient and Hessian-vector product in 32-sample chunks); a workgroup
// whose index is beyond a pass's chunk count only waits at that pass's barrier.  Three exchanges per step (two when
// first order), slots alternate by exchange parity.  Every workgroup applies the same Adam update to its own copy of
// theta; the moments of workgroup w > 0 are private copies in the workspace (`moments`), workgroup 0 works on the
// caller's adam_m / adam_v.
template <int SC, bool MANY>
__global__ __launch_bounds__(kTrainThreads) void maml_train_groups_kernel(
    const mvn_train_trial_t one, const mvn_train_trial_t *__restrict__ many, int T, int W, float meta_lr, int second_order,
    float lr, float beta1, float beta2, float eps, int S_rt, int lds_floats, const GroupLaunch gl) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float s_step_size, s_inv_sqrt_bc2;
    const GroupPlace pl = group_place(gl);
    if (!pl.active) return;
    const mvn_train_trial_t &d = MANY ? many[pl.trial] : one;
    const int n_steps = d.n;
    if (n_steps <= 0) return;  // the whole trial: all its workgroups leave before any barrier
    const float *__restrict__ rx_words = d.y;
    const int *__restrict__ labels = d.labels, *__restrict__ support_idx = d.idx, *__restrict__ query_idx = d.query_idx;
    float *__restrict__ adam_m = d.adam_m, *__restrict__ adam_v = d.adam_v, *__restrict__ loss_out = d.loss_out;
    double b1pow = d.b1pow, b2pow = d.b2pow;
    const int S = SC ? SC : S_rt;
    const TrainLayout L = train_layout(S);
    float *th = smem, *ga = th + L.P4, *gq = ga + L.P4, *thp = gq + L.P4, *arena = thp + L.P4;  // as in maml_train_kernel
    const ChunkArena<kTrainChunk> A(arena);
    const HvArena<kHvRows> HA(thp);  // theta' is dead by the Hessian pass
    const int tid = threadIdx.x, w = pl.w, G = pl.G;
    float *workspace = gl.workspace + (MANY ? (long long)pl.trial * gl.ws_stride : 0);
    GroupSync *gs = reinterpret_cast<GroupSync *>(workspace);
    SlotIO io(workspace, gl.ws_bytes);
    const size_t slots = sizeof(GroupSync) / sizeof(float);  // float offset of the slots in the trial's region
    const size_t X = train_group_slot_floats(S);
    const unsigned n_arrive = (unsigned)(G + (gl.phantoms > 0 ? gl.phantoms : 0));
    const bool skip_tag = gl.phantoms < 0 && w == -gl.phantoms - 1;  // test hook: this workgroup never publishes its tag
    announce_xcd(gs);
    // private copies of the moments (workgroup w > 0): read and written by their owner only, plain accesses
    float *mom_m = w == 0 ? adam_m : workspace + slots + (size_t)2 * G * X + (size_t)(w - 1) * 2 * L.Pflat;
    float *mom_v = w == 0 ? adam_v : mom_m + L.Pflat;

    MVN_CLEAR_LDS_LOAD_PARAMS(kTrainThreads, th);
    if (w != 0)
        for (int e = tid; e < L.Pflat; e += kTrainThreads) {  // thread e owns moment e from here to the end
            mom_m[e] = adam_m[e];
            mom_v[e] = adam_v[e];
        }
    unsigned epoch = 0, xchg = 0;
    bool good = groups_barrier(gs, n_arrive, epoch, gl.spin_limit);  // nobody updates adam_m / adam_v before everybody has its copy
    set_same_xcd(io, gs, good, gl.groups > 0 && gl.phantoms <= 0);

    const int n_sup = W * T, n_qry = T;
    const int sup_chunks = (n_sup + kTrainChunk - 1) / kTrainChunk, qry_chunks = (n_qry + kTrainChunk - 1) / kTrainChunk;
    const int hv_chunks = (n_sup + kHvRows - 1) / kHvRows;
    const float inv_ns = 1.0f / (float)n_sup, inv_nq = 1.0f / (float)n_qry;
    auto clear_pads_grad = [&]() {
        for (int e = tid; e < kTrainChunk * 2; e += kTrainThreads) {
            const int i = (e >> 1) * kZ2Stride + kH2 + (e & 1);
            A.z2[i] = 0.0f;
            A.dz2[i] = 0.0f;
        }
        for (int e = tid; e < kTrainChunk * kDlStride; e += kTrainThreads)
            if (e % kDlStride >= S) A.dl[e] = 0.0f;
    };
    auto clear_pads_hv = [&]() {
        for (int e = tid; e < kHvRows * 2; e += kTrainThreads) {
            const int i = (e >> 1) * kZ2Stride + kH2 + (e & 1);
            HA.z2[i] = 0.0f;
            HA.Ra2[i] = 0.0f;
            HA.dz2[i] = 0.0f;
            HA.Rdz2[i] = 0.0f;
        }
        for (int e = tid; e < kHvRows * kDlStride; e += kTrainThreads)
            if (e % kDlStride >= S) {
                HA.dlo[e] = 0.0f;
                HA.Rdo[e] = 0.0f;
            }
    };
    const MetaSamples smp = {support_idx, query_idx, W, T};
    // this workgroup's vector `vec` (float4 e4 owned by thread e4 after a chunk call) -> its slot of the next exchange
    auto publish = [&](const float *vec, float extra) {
        const size_t mine = slots + ((size_t)(xchg & 1) * G + w) * X;
        for (int e4 = tid; e4 < L.P4 / 4; e4 += kTrainThreads) io.store4(mine + 4 * (size_t)e4, reinterpret_cast<const float4 *>(vec)[e4]);
        if (tid == 0) io.store1(mine + L.P4, extra);
    };

    // Samples of this workgroup's chunks, fetched one step ahead by threads < 32: the index -> sample round trips (two dependent
    // global loads per pass) hide behind the previous step's work.  The Hessian pass's chunk w holds the same samples as the
    // support pass's (kHvRows == kTrainChunk), and the two labels of a thread (5-bit trellis states) share one register: three
    // registers live across a step's chunk calls for the step after it, and this step's samples wait in LDS (s_cur), not in
    // registers -- the kernel sits at the 128-register limit of a 1024-thread workgroup.
    static_assert(kHvRows == kTrainChunk, "the Hessian pass reuses the support pass's samples");
    __shared__ float s_cur_y[2][kTrainChunk];
    __shared__ int s_cur_lab[kTrainChunk];
    struct StepSamples {
        float ys, yq;
        int labs;  // support label | query label << 8
    } nxt = {0.f, 0.f, 0};
    auto fetch_step = [&](int step) {
        StepSamples r = {0.f, 0.f, 0};
        if (tid < kTrainChunk && step < n_steps) {
            const int ns = w * kTrainChunk + tid;
            if (w < sup_chunks && ns < n_sup) {
                const long long s_ = smp.support(step, ns);
                r.ys = rx_words[s_];
                r.labs = labels[s_];
            }
            if (w < qry_chunks && ns < n_qry) {
                const long long s_ = smp.query(step, ns);
                r.yq = rx_words[s_];
                r.labs |= labels[s_] << 8;
            }
        }
        return r;
    };
    nxt = fetch_step(0);
    for (int step = 0; step < n_steps && good; ++step) {
        if (tid < kTrainChunk) {  // this step's samples (rows >= the chunk's count were fetched as zeros); read after a barrier
            s_cur_y[0][tid] = nxt.ys;
            s_cur_y[1][tid] = nxt.yq;
            s_cur_lab[tid] = nxt.labs;
        }
        nxt = fetch_step(step + 1);
        if (tid == kTrainThreads - 1) next_bias_corrections<true>(b1pow, b2pow, lr, beta1, beta2, s_step_size, s_inv_sqrt_bc2);
        // ---- pass 0: g_s = grad L_support(theta), chunk w -> slot, theta' = theta - meta_lr sum of the slots;
        //      pass 1: g_q = grad L_query(theta'), chunk w -> slot, sum -> gq.  One loop over the passes with the pass's parameters
        //      always in `th` and its gradient in `ga` (theta waits in `thp` during the query pass): one inlined copy of the chunk
        //      code per form, every LDS address an immediate -- as in maml_train_kernel.
        float loss_q = 0.0f;
        for (int pass = 0; pass < 2; ++pass) {
            const int chunks = pass ? qry_chunks : sup_chunks, n_pass = pass ? n_qry : n_sup;
            if (w < chunks) {
                // (float4 tid and tid + 1024: the elements this thread itself read in the previous exchange's sum_slots -- no other
                // thread's read of its own vector can still be outstanding, so no barrier is needed in front of this)
                reinterpret_cast<float4 *>(ga)[tid] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (tid + kTrainThreads < L.P4 / 4) reinterpret_cast<float4 *>(ga)[tid + kTrainThreads] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (pass && tid == 0) A.red[kTrainChunk] = 0.0f;
                if (pass == 0 || w >= sup_chunks) clear_pads_grad();
                const int c0 = w * kTrainChunk, nc = n_pass - c0 < kTrainChunk ? n_pass - c0 : kTrainChunk;
                if (tid < kTrainChunk) {  // rows >= nc were fetched as zeros
                    A.ys[tid] = s_cur_y[pass][tid];
                    A.lab[tid] = (s_cur_lab[tid] >> (8 * pass)) & 255;
                }
                __syncthreads();
                if (w > 0 && nc <= 16) grad_chunk<16, false>(th, ga, L, A, nc, pass ? inv_nq : inv_ns, S);  // (chunk 0: always the full form)
                else grad_chunk<kTrainChunk, false>(th, ga, L, A, nc, pass ? inv_nq : inv_ns, S);
                publish(ga, pass ? A.red[kTrainChunk] : 0.0f);
            }
            good = groups_barrier(gs, n_arrive, epoch, gl.spin_limit, io.same_xcd, 1, w, skip_tag) && good;  // (the moment-copy barrier's failure is sticky too)
            const size_t all = slots + (size_t)(xchg & 1) * G * X;
            float4 tot[2];
            sum_slots(io, all, X, chunks, tid, L.P4 / 4, tot, w < chunks ? w : -1, ga);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int e4 = tid + j * kTrainThreads;
                if (e4 >= L.P4 / 4) break;
                if (pass) {  // g_q, and theta back in its place
                    reinterpret_cast<float4 *>(gq)[e4] = tot[j];
                    reinterpret_cast<float4 *>(th)[e4] = reinterpret_cast<const float4 *>(thp)[e4];
                } else {  // theta -> thp, theta' -> th
                    const float4 gs4 = tot[j], t4 = reinterpret_cast<const float4 *>(th)[e4];
                    reinterpret_cast<float4 *>(thp)[e4] = t4;
                    reinterpret_cast<float4 *>(th)[e4] = make_float4(t4.x - meta_lr * gs4.x, t4.y - meta_lr * gs4.y, t4.z - meta_lr * gs4.z, t4.w - meta_lr * gs4.w);
                }
            }
            if (pass && w == 0 && tid == 0) {
                loss_q = io.load1(all + L.P4);
                for (int c = 1; c < qry_chunks; ++c) loss_q += io.load1(all + c * X + L.P4);
                loss_q *= inv_nq;
            }
            ++xchg;
        }
        __syncthreads();  // gq complete: the Hessian pass reads it as the direction, Adam as the gradient
        // ---- H_support(theta) g_q: chunk w -> slot; sum -> ga
        if (second_order) {
            if (w < hv_chunks) {
                for (int e = tid; e < L.P4; e += kTrainThreads) ga[e] = 0.0f;
                clear_pads_hv();
                const int c0 = w * kHvRows, nc = n_sup - c0 < kHvRows ? n_sup - c0 : kHvRows;
                if (tid < kHvRows) {
                    HA.ys[tid] = s_cur_y[0][tid];
                    HA.lab[tid] = s_cur_lab[tid] & 255;
                }
                __syncthreads();
                if (nc <= 16) hv_chunk<16>(th, gq, ga, L, HA, nc, inv_ns, S);
                else hv_chunk<kHvRows>(th, gq, ga, L, HA, nc, inv_ns, S);
                publish(ga, 0.0f);
            }
            good = groups_barrier(gs, n_arrive, epoch, gl.spin_limit, io.same_xcd, 1, w, skip_tag) && good;
            const size_t all = slots + (size_t)(xchg & 1) * G * X;
            float4 tot[2];
            sum_slots(io, all, X, hv_chunks, tid, L.P4 / 4, tot, w < hv_chunks ? w : -1, ga);
            reinterpret_cast<float4 *>(ga)[tid] = tot[0];
            if (tid + kTrainThreads < L.P4 / 4) reinterpret_cast<float4 *>(ga)[tid + kTrainThreads] = tot[1];
            ++xchg;
            __syncthreads();
        }
        // ---- theta <- Adam(theta, g_q - meta_lr H g_q), identically in every workgroup
        const float step_size = s_step_size, inv_sqrt_bc2 = s_inv_sqrt_bc2;
        for (int e = tid; e < L.Pflat; e += kTrainThreads) {
            const int le = lds_index(e);
            const float gr = second_order ? gq[le] - meta_lr * ga[le] : gq[le];
            float pe = th[le], me = mom_m[e], ve = mom_v[e];
            adam1(pe, me, ve, gr, beta1, beta2, eps, step_size, inv_sqrt_bc2);
            th[le] = pe;
            mom_m[e] = me;
            mom_v[e] = ve;
        }
        if (w == 0 && tid == 0 && loss_out) loss_out[step] = loss_q;
        __syncthreads();
    }
    if (w != 0) return;
    MVN_FINISH_GROUP_TRIAL(th);
}

inline size_t maml_groups_workspace_bytes(int S, int groups) {
    return train_groups_workspace_bytes(S, groups) + (size_t)(groups - 1) * 2 * train_layout(S).Pflat * sizeof(float);
}
