// jax_raft_amd native runtime: the plan executor.  A Plan knows no op: binding.cpp
// turns checked arguments into launch closures and records them with Plan::add.
#pragma once
#include <torch/custom_class.h>
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>
#include <rocprofiler-sdk-roctx/roctx.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <unordered_map>
#include <vector>

namespace jr {


using Launch = std::function<int(hipStream_t, int)>;

static inline hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

#define JR_CHECK_OK(expr)                                                                 \
  do {                                                                                    \
    int e__ = (expr);                                                                     \
    TORCH_CHECK(e__ == 0, "jax_raft_amd kernel launch failed: ", hipGetErrorString((hipError_t)e__)); \
  } while (0)

// --------------------------------------------------------------------- Plan
// A Plan is the lowered RAFT forward: three segments (prologue, loop body run
// n_iters times with the iteration index, epilogue) of launch closures.  Ops
// are placed on "lanes": lane 0 is the caller's stream, lanes 1..kMaxLanes-1
// are private non-blocking streams, and record/wait ops on numbered events
// express the cross-lane dependencies of the model's DAG (independent
// branches such as the context encoder vs. the feature encoder + correlation
// pyramid, or the mask head + upsampling of iteration i vs. iteration i+1).
// Every side lane is forked from lane 0 at the start of an enqueue and joined
// back at its end, so run() is ordered like a single-stream launch and
// capture() records one hipGraph whose parallel branches the runtime may
// execute concurrently.  A wait on an event not yet recorded during the
// current enqueue is skipped (e.g. the first iteration's wait on the previous
// iteration's mask head), which also keeps graph capture self-contained.
// Lane 0 runs on a private stream of the device's greatest priority (forked
// from / joined to the caller's stream): the model's critical path (lookup ->
// motion encoder -> GRU -> flow head) wins the dispatcher over the side lanes'
// work, which only fills the CUs the critical path leaves idle.
struct RangeGuard {
  explicit RangeGuard(const char* name) { roctxRangePushA(name); }
  ~RangeGuard() { roctxRangePop(); }
};

class Plan : public torch::CustomClassHolder {
 public:
  static constexpr int kMaxLanes = 8;
  static constexpr int kMaxEvents = 64;
  Plan() = default;
  ~Plan() override {
    reset_graph();
    for (auto e : events_) if (e) (void)hipEventDestroy(e);
    for (auto e : join_) if (e) (void)hipEventDestroy(e);
    if (fork_) (void)hipEventDestroy(fork_);
    for (auto st : lanes_) if (st) (void)hipStreamDestroy(st);
    if (cap_stream_) (void)hipStreamDestroy(cap_stream_);
  }

  // Segment 3 is the second half of the loop body (enqueued right after segment 1 in
  // every iteration): a context-parallel engine runs the two halves separately, with
  // the all-gather of the correlation features in between (run_segment).
  void set_segment(int64_t s) {
    TORCH_CHECK(s >= 0 && s <= 3, "segment must be 0 (prologue), 1 (loop), 2 (epilogue) or 3 (loop, second half)");
    seg_ = (int)s;
    defer_ = 0;
    reset_graph();
  }
  // Deferred ops (set_defer 1, loop body / epilogue): the work of the PREVIOUS
  // iteration -- skipped in loop iteration 0 and called with iteration index
  // it - 1; in the epilogue (called with n_iters) they finish the last
  // iteration.  Used when iteration i's flow update is fused into iteration
  // i+1's lookup, so iteration i's mask head / upsampling run one iteration later.
  void set_defer(int64_t d) {
    TORCH_CHECK(d == 0 || d == 1, "defer must be 0 or 1");
    TORCH_CHECK(d == 0 || seg_ != 0, "deferred ops belong to the loop body or the epilogue");
    defer_ = (int)d;
  }
  void set_lane(int64_t l) {
    TORCH_CHECK(l >= 0 && l < kMaxLanes, "lane must be in [0, ", kMaxLanes, ")");
    lane_ = (int)l;
    used_lanes_ = std::max(used_lanes_, lane_ + 1);
  }
  void add_record(int64_t ev) { push_sync(OP_RECORD, ev, "record"); }
  void add_wait(int64_t ev) { push_sync(OP_WAIT, ev, "wait"); }
  // Record one launch in the current segment / lane (the Plan.add_<op> methods that binding.cpp
  // generates from its op table).  keep(): the tensors a launch points into live as long as the plan.
  void add(Launch l, const char* name) { push(std::move(l), name); }
  std::vector<at::Tensor>& keep() { return keep_; }

  int64_t num_ops(int64_t seg) const { return (int64_t)segs_[seg].size(); }
  std::vector<std::string> op_names(int64_t seg) const {
    std::vector<std::string> out;
    for (const auto& o : segs_[seg]) out.push_back(o.name + (o.lane ? "@" + std::to_string(o.lane) : std::string()));
    return out;
  }
  int64_t num_lanes() const { return used_lanes_; }

  // Launch prologue, n_iters x loop body, epilogue (lane 0 = current stream).
  void run(int64_t n_iters) { JR_CHECK_OK(enqueue(cur_stream(), (int)n_iters)); }
  // Launch one segment alone with iteration index `it` (eager; host-driven loops
  // that interleave collectives with the segments, runtime/engine.py context parallelism).
  void run_segment(int64_t seg, int64_t it) {
    TORCH_CHECK(seg >= 0 && seg <= 3, "segment must be 0..3");
    JR_CHECK_OK(enqueue(cur_stream(), (int)it, false, -1, (int)seg));
  }
  // Enqueue into a stream that an outer capture is recording (e.g. a whole
  // training step captured by torch.cuda.graph): lane 0 is the caller's stream
  // itself, as in capture(), so the origin stream never holds only fork / join
  // event nodes (which crashes hipStreamEndCapture on this ROCm); no per-op
  // checks (no synchronisation inside a capture).
  void run_inline(int64_t n_iters) { JR_CHECK_OK(enqueue(cur_stream(), (int)n_iters, true)); }

  // Capture the same sequence into one hipGraph (on a private stream: the
  // legacy default stream cannot be captured) and instantiate it.
  void capture(int64_t n_iters) {
    reset_graph();
    capture_into(n_iters, -1, &graph_, &exec_);
    captured_iters_ = n_iters;
  }
  // Capture one phase as its own hipGraph: part 0 = the prologue (encoders +
  // correlation pyramid), part 1 = n_iters loop iterations + the epilogue.
  // Replayed on different streams, the prologue of batch i+1 overlaps the
  // refinement loop of batch i (cross-batch pipelining, runtime/engine.py).
  void capture_part(int64_t part, int64_t n_iters) {
    TORCH_CHECK(part == 0 || part == 1, "part must be 0 (prologue) or 1 (loop + epilogue)");
    reset_part(part);
    capture_into(n_iters, (int)part, &pgraph_[part], &pexec_[part]);
    pcaptured_[part] = n_iters;
  }
  int64_t captured_part_iters(int64_t part) const { return pcaptured_[part & 1]; }
  void replay_part(int64_t part) {
    TORCH_CHECK((part == 0 || part == 1) && pexec_[part] != nullptr, "plan: part ", part, " not captured");
    hipError_t e = hipGraphLaunch(pexec_[part], cur_stream());
    TORCH_CHECK(e == hipSuccess, "graph launch failed: ", hipGetErrorString(e));
  }

  // Software-pipelined step: ONE hipGraph holding this plan's refinement loop
  // + epilogue (batch i) and `next`'s prologue (encoders + correlation pyramid
  // of batch i+1, a plan with its own buffers) as independent branches.  The
  // loop is latency-bound (one workgroup per CU, ~220 of 256 CUs per kernel);
  // the throughput-bound encoder convs fill the idle SIMD slots.  Two graphs
  // launched on two streams serialise on this ROCm (measured 196 pairs/s,
  // engine.submit), the branches of one graph do not.  The loop branch is
  // enqueued first, so its nodes come first in the graph's launch order.
  void capture_pipelined(c10::intrusive_ptr<Plan> next, int64_t n_iters) {
    TORCH_CHECK(next.get() != this, "capture_pipelined: the next plan must have its own buffers");
    reset_pipe();
    // The two phases are captured on their own (capture_part) and their nodes
    // copied, with their dependency edges, into one graph with no edge between
    // the two: every lane of both stays a parallel branch.  (Enqueueing both
    // into one stream capture -- the next plan's lanes forked from this one's
    // capture stream -- crashed hipStreamEndCapture on this ROCm whenever both
    // plans use several lanes (batch 4); a child-graph node runs its graph's
    // nodes in order on one stream, i.e. without the lanes.)
    if (pcaptured_[1] != n_iters) capture_part(1, n_iters);
    if (next->pcaptured_[0] != n_iters) next->capture_part(0, n_iters);
    debug_ = std::getenv("JR_PLAN_DEBUG") != nullptr;
    hipGraph_t g = nullptr;
    TORCH_CHECK(hipGraphCreate(&g, 0) == hipSuccess, "graph create");
    pipe_graph_ = g;
    // loop nodes first (the executor launches in creation order; the prologue's first
    // measured batch 1 157 -> 78 pairs/s, the two phases then run one after the other).
    // (The prologue as one child-graph node, i.e. its nodes in order on one stream,
    // measured 264 vs 289 pairs/s at batch 4.)
    // One empty root node ahead of both branches: the executor forks a node's successors
    // onto parallel streams, but runs disconnected components in creation order on the
    // launch stream (measured: 21.6 us of a 3.2 ms raft_small batch-1 step concurrent;
    // with the root raft_small b1 12 it 788 vs 713 pairs/s, profiles/r5_pipeline_fork_ab.txt).
    hipGraphNode_t root = nullptr;
    TORCH_CHECK(hipGraphAddEmptyNode(&root, g, nullptr, 0) == hipSuccess, "graph root");
    append_graph(g, pgraph_[1], root);
    append_graph(g, next->pgraph_[0], root);
    hipError_t e3 = hipGraphInstantiate(&pipe_exec_, g, nullptr, nullptr, 0);
    if (debug_) fprintf(stderr, "[plan] pipelined instantiate %d\n", (int)e3);
    TORCH_CHECK(e3 == hipSuccess, "graph instantiate failed: ", hipGetErrorString(e3));
    pipe_iters_ = n_iters;
    pipe_next_ = next.get();
  }
  // Copy every node of src (kernel / empty nodes: what a plan capture holds)
  // into dst in dependency order, keeping src's edges.
  static void append_graph(hipGraph_t dst, hipGraph_t src, hipGraphNode_t root = nullptr) {
    size_t n = 0;
    TORCH_CHECK(hipGraphGetNodes(src, nullptr, &n) == hipSuccess, "graph nodes");
    std::vector<hipGraphNode_t> nodes(n);
    TORCH_CHECK(hipGraphGetNodes(src, nodes.data(), &n) == hipSuccess, "graph nodes");
    std::unordered_map<hipGraphNode_t, size_t> index;
    for (size_t i = 0; i < n; ++i) index[nodes[i]] = i;
    std::vector<std::vector<size_t>> deps(n), users(n);
    std::vector<size_t> missing(n, 0);
    for (size_t i = 0; i < n; ++i) {
      size_t nd = 0;
      TORCH_CHECK(hipGraphNodeGetDependencies(nodes[i], nullptr, &nd) == hipSuccess, "node deps");
      std::vector<hipGraphNode_t> d(nd);
      if (nd) TORCH_CHECK(hipGraphNodeGetDependencies(nodes[i], d.data(), &nd) == hipSuccess, "node deps");
      for (auto x : d) {
        const size_t j = index.at(x);
        deps[i].push_back(j);
        users[j].push_back(i);
      }
      missing[i] = deps[i].size();
    }
    std::vector<hipGraphNode_t> copy(n, nullptr);
    // ready nodes are copied in src creation order: the executor maps a node's
    // successors onto its streams in creation order, and a depth-first copy of
    // the forward graph measured 6 % slower (profiles/r2_pipelined_graph_ab.txt)
    std::vector<size_t> ready;
    for (size_t i = 0; i < n; ++i) if (!missing[i]) ready.push_back(i);
    size_t done = 0;
    while (!ready.empty()) {
      const auto it = std::min_element(ready.begin(), ready.end());
      const size_t i = *it;
      ready.erase(it);
      std::vector<hipGraphNode_t> d;
      for (size_t j : deps[i]) d.push_back(copy[j]);
      if (d.empty() && root) d.push_back(root);
      hipGraphNodeType type;
      TORCH_CHECK(hipGraphNodeGetType(nodes[i], &type) == hipSuccess, "node type");
      hipError_t e = hipSuccess;
      if (type == hipGraphNodeTypeKernel) {
        hipKernelNodeParams kp;
        e = hipGraphKernelNodeGetParams(nodes[i], &kp);
        if (e == hipSuccess) e = hipGraphAddKernelNode(&copy[i], dst, d.data(), d.size(), &kp);
      } else if (type == hipGraphNodeTypeEmpty) {
        e = hipGraphAddEmptyNode(&copy[i], dst, d.data(), d.size());
      } else {
        TORCH_CHECK(false, "capture_pipelined: unsupported graph node type ", (int)type);
      }
      TORCH_CHECK(e == hipSuccess, "capture_pipelined: node copy failed: ", hipGetErrorString(e));
      ++done;
      for (size_t u : users[i]) if (--missing[u] == 0) ready.push_back(u);
    }
    TORCH_CHECK(done == n, "capture_pipelined: cyclic graph");
  }
  // Batch parts as ONE graph: every part plan's full-forward capture (own
  // buffers, own lanes) copied into a single graph with no edge between the
  // parts, so their in-order chains interleave on the GPU without any
  // cross-stream edge (separate graphs on separate streams serialise on this
  // ROCm).  merge_reset(); merge_add(part) for every part; merge_finish(n);
  // replay_pipelined().
  void merge_reset() {
    reset_pipe();
    TORCH_CHECK(hipGraphCreate(&pipe_graph_, 0) == hipSuccess, "graph create");
    // one root: the parts fork (capture_pipelined)
    TORCH_CHECK(hipGraphAddEmptyNode(&pipe_root_, pipe_graph_, nullptr, 0) == hipSuccess, "graph root");
  }
  void merge_add(c10::intrusive_ptr<Plan> part, int64_t n_iters) {
    TORCH_CHECK(pipe_graph_ != nullptr && pipe_exec_ == nullptr, "merge_add: call merge_reset() first");
    if (part->captured_iters_ != n_iters) {
      // capture() resets this plan's graphs, the merge in progress included
      hipGraph_t merging = pipe_graph_;
      pipe_graph_ = nullptr;
      part->capture(n_iters);
      pipe_graph_ = merging;
    }
    append_graph(pipe_graph_, part->graph_, pipe_root_);
  }
  void merge_finish(int64_t n_iters) {
    TORCH_CHECK(pipe_graph_ != nullptr && pipe_exec_ == nullptr, "merge_finish: call merge_reset() first");
    hipError_t e = hipGraphInstantiate(&pipe_exec_, pipe_graph_, nullptr, nullptr, 0);
    TORCH_CHECK(e == hipSuccess, "graph instantiate failed: ", hipGetErrorString(e));
    pipe_iters_ = n_iters;
    pipe_next_ = this;
  }
  int64_t merged_iters() const { return pipe_next_ == this ? pipe_iters_ : -1; }

  // n_iters of the pipelined graph if it was captured with `next`, else -1.
  int64_t pipelined_iters(c10::intrusive_ptr<Plan> next) const {
    return pipe_next_ == next.get() ? pipe_iters_ : -1;
  }
  void replay_pipelined() {
    TORCH_CHECK(pipe_exec_ != nullptr, "plan: no pipelined graph captured");
    hipError_t e = hipGraphLaunch(pipe_exec_, cur_stream());
    TORCH_CHECK(e == hipSuccess, "graph launch failed: ", hipGetErrorString(e));
  }

 private:
  void reset_pipe() {
    if (pipe_exec_) { (void)hipGraphExecDestroy(pipe_exec_); pipe_exec_ = nullptr; }
    if (pipe_graph_) { (void)hipGraphDestroy(pipe_graph_); pipe_graph_ = nullptr; }
    pipe_root_ = nullptr;
    pipe_iters_ = -1;
    pipe_next_ = nullptr;
  }
  hipStream_t ensure_cap_stream() {
    if (!cap_stream_) {
      int least = 0, greatest = 0;
      TORCH_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess, "priority range");
      TORCH_CHECK(hipStreamCreateWithPriority(&cap_stream_, hipStreamNonBlocking, greatest) == hipSuccess, "stream");
    }
    return cap_stream_;
  }
  void reset_part(int64_t part) {
    if (pexec_[part]) { (void)hipGraphExecDestroy(pexec_[part]); pexec_[part] = nullptr; }
    if (pgraph_[part]) { (void)hipGraphDestroy(pgraph_[part]); pgraph_[part] = nullptr; }
    pcaptured_[part] = -1;
  }
  void capture_into(int64_t n_iters, int part, hipGraph_t* graph_out, hipGraphExec_t* exec_out) {
    hipStream_t s = ensure_cap_stream();
    debug_ = std::getenv("JR_PLAN_DEBUG") != nullptr;
    // order the capture after work already queued on the current stream
    TORCH_CHECK(hipStreamSynchronize(cur_stream()) == hipSuccess, "sync");
    TORCH_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) == hipSuccess, "begin capture");
    int err = enqueue(s, (int)n_iters, true, part);
    if (debug_) fprintf(stderr, "[plan] enqueue done err=%d\n", err);
    hipGraph_t g = nullptr;
    hipError_t e2 = hipStreamEndCapture(s, &g);
    if (debug_) fprintf(stderr, "[plan] end capture %d\n", (int)e2);
    TORCH_CHECK(err == 0, "launch failed during capture: ", hipGetErrorString((hipError_t)err));
    TORCH_CHECK(e2 == hipSuccess && g != nullptr, "end capture failed: ", hipGetErrorString(e2));
    *graph_out = g;
    hipError_t e3 = hipGraphInstantiate(exec_out, g, nullptr, nullptr, 0);
    if (debug_) fprintf(stderr, "[plan] instantiate %d\n", (int)e3);
    TORCH_CHECK(e3 == hipSuccess, "graph instantiate failed: ", hipGetErrorString(e3));
  }

 public:
  int64_t captured_iters() const { return captured_iters_; }
  void replay() {
    TORCH_CHECK(exec_ != nullptr, "plan: no captured graph");
    hipError_t e = hipGraphLaunch(exec_, cur_stream());
    TORCH_CHECK(e == hipSuccess, "graph launch failed: ", hipGetErrorString(e));
  }
  void reset_graph() {
    if (exec_) { (void)hipGraphExecDestroy(exec_); exec_ = nullptr; }
    if (graph_) { (void)hipGraphDestroy(graph_); graph_ = nullptr; }
    captured_iters_ = -1;
    reset_part(0);
    reset_part(1);
    reset_pipe();
  }

 private:
  enum OpKind { OP_LAUNCH = 0, OP_RECORD = 1, OP_WAIT = 2 };
  struct Op {
    Launch l;
    int lane;
    int kind;
    int ev;
    std::string name;
    int defer;   // 1: previous iteration's work (see set_defer)
  };
  void push(Launch l, const char* name) {
    segs_[seg_].push_back(Op{std::move(l), lane_, OP_LAUNCH, -1, name, defer_});
    reset_graph();
  }
  void push_sync(int kind, int64_t ev, const char* name) {
    TORCH_CHECK(ev >= 0 && ev < kMaxEvents, "event id out of range");
    segs_[seg_].push_back(Op{Launch(), lane_, kind, (int)ev, std::string(name) + std::to_string(ev), defer_});
    reset_graph();
  }
  static int create_event(hipEvent_t* e) {
    return (int)hipEventCreateWithFlags(e, hipEventDisableTiming);
  }
  int ensure_resources() {
    if (events_.empty()) {
      events_.assign(kMaxEvents, nullptr);
      for (auto& e : events_) if (int r = create_event(&e)) return r;
    }
    if (!fork_) if (int r = create_event(&fork_)) return r;
    int least = 0, greatest = 0;
    if (int r = (int)hipDeviceGetStreamPriorityRange(&least, &greatest)) return r;
    if (!lanes_[0]) if (int r = (int)hipStreamCreateWithPriority(&lanes_[0], hipStreamNonBlocking, greatest)) return r;
    if (!join_[0]) if (int r = create_event(&join_[0])) return r;
    for (int l = 1; l < used_lanes_; ++l) {
      if (!lanes_[l]) if (int r = (int)hipStreamCreateWithPriority(&lanes_[l], hipStreamNonBlocking, least)) return r;
      if (!join_[l]) if (int r = create_event(&join_[l])) return r;
    }
    return 0;
  }
  // recorded[ev] = 1 + lane of the event's latest record in this enqueue (0: not recorded).
  // A wait on an event last recorded on the same lane is already satisfied by stream
  // order and is skipped (a same-stream record/wait pair on a forked capture stream
  // also crashes hipStreamEndCapture on this ROCm).
  int exec_op(const Op& o, hipStream_t* st, int it, std::vector<char>& recorded) {
    if (o.defer) {
      if (it == 0) return 0;
      --it;
    }
    hipStream_t s = st[o.lane];
    if (debug_) fprintf(stderr, "[plan] it=%d lane=%d %s stream=%p\n", it, o.lane, o.name.c_str(), (void*)s);
    switch (o.kind) {
      case OP_LAUNCH: {
        const int r = o.l(s, it);
        // JR_PLAN_CHECK=1 (eager run only): synchronise after every launch so an asynchronous
        // fault or launch error is attributed to the op that caused it (fault localisation,
        // SURVEY.md 5.2); the failing op's segment index, lane, iteration and name are reported.
        if (check_ && !capturing_) {
          hipError_t e = r ? (hipError_t)r : hipStreamSynchronize(s);
          if (e == hipSuccess) e = hipGetLastError();
          if (e != hipSuccess) {
            fprintf(stderr, "[plan check] op '%s' (lane %d, iteration %d) failed: %s\n", o.name.c_str(), o.lane, it,
                    hipGetErrorString(e));
            return (int)e;
          }
        }
        return r;
      }
      case OP_RECORD: recorded[o.ev] = (char)(1 + o.lane); return (int)hipEventRecord(events_[o.ev], s);
      default:
        if (!recorded[o.ev] || recorded[o.ev] == 1 + o.lane) return 0;
        return (int)hipStreamWaitEvent(s, events_[o.ev], 0);
    }
  }
  // part: -1 = the whole forward, 0 = prologue only, 1 = loop + epilogue only.
  // only_seg >= 0: just that segment, with iteration index n_iters.
  int enqueue(hipStream_t s, int n_iters, bool capturing = false, int part = -1, int only_seg = -1) {
    if (int r = ensure_resources()) return r;
    check_ = std::getenv("JR_PLAN_CHECK") != nullptr && std::getenv("JR_PLAN_CHECK")[0] == '1';
    capturing_ = capturing;
    // Eager: lane 0 is the private high-priority stream, forked from the caller's.
    // Capture: lane 0 is the capture stream itself (created with the greatest
    // priority); a capture whose origin stream holds only the fork/join event
    // nodes crashes hipStreamEndCapture on this ROCm.
    const int l0 = capturing ? 1 : 0;
    hipStream_t st[kMaxLanes] = {};
    st[0] = s;
    // fork / join only the lanes that hold ops in the enqueued segments: a forked
    // capture stream holding nothing but the fork wait and the join record
    // crashes hipStreamEndCapture on this ROCm (e.g. the context-encoder lane in
    // a loop-only capture, capture_part(1))
    bool used[kMaxLanes] = {};
    used[0] = true;
    for (int sg = 0; sg < 4; ++sg) {
      if ((sg == 0 && part == 1) || (sg != 0 && part == 0)) continue;
      if (only_seg >= 0 && sg != only_seg) continue;
      for (const auto& o : segs_[sg]) used[o.lane] = true;
    }
    if (int r = (int)hipEventRecord(fork_, s)) return r;
    for (int l = l0; l < used_lanes_; ++l) {
      if (!used[l]) continue;
      st[l] = lanes_[l];
      if (int r = (int)hipStreamWaitEvent(st[l], fork_, 0)) return r;
    }
    std::vector<char> recorded(kMaxEvents, 0);
    // roctx ranges (visible in rocprofv3 --marker-trace) bracket the host-side
    // enqueue of each phase: encoders + correlation pyramid, every refinement
    // iteration, the epilogue.
    RangeGuard all("raft.plan");
    if (only_seg >= 0) {
      RangeGuard r("raft.segment");
      for (auto& o : segs_[only_seg]) if (int e = exec_op(o, st, n_iters, recorded)) return e;
    } else {
    if (part != 1) {
      RangeGuard r("raft.prologue");
      for (auto& o : segs_[0]) if (int e = exec_op(o, st, 0, recorded)) return e;
    }
    for (int it = 0; part != 0 && it < n_iters; ++it) {
      RangeGuard r("raft.iteration");
      for (auto& o : segs_[1]) if (int e = exec_op(o, st, it, recorded)) return e;
      for (auto& o : segs_[3]) if (int e = exec_op(o, st, it, recorded)) return e;
    }
    if (part != 0) {
      RangeGuard r("raft.epilogue");
      for (auto& o : segs_[2]) if (int e = exec_op(o, st, n_iters, recorded)) return e;
    }
    }
    for (int l = l0; l < used_lanes_; ++l) {
      if (!used[l]) continue;
      if (int r = (int)hipEventRecord(join_[l], st[l])) return r;
      if (int r = (int)hipStreamWaitEvent(s, join_[l], 0)) return r;
    }
    return 0;
  }
  std::vector<Op> segs_[4];
  std::vector<at::Tensor> keep_;
  int seg_ = 0;
  int lane_ = 0;
  int defer_ = 0;
  int used_lanes_ = 1;
  std::vector<hipEvent_t> events_;
  hipEvent_t fork_ = nullptr;
  hipEvent_t join_[kMaxLanes] = {};
  hipStream_t lanes_[kMaxLanes] = {};
  hipStream_t cap_stream_ = nullptr;
  hipGraph_t graph_ = nullptr;
  hipGraphExec_t exec_ = nullptr;
  int64_t captured_iters_ = -1;
  hipGraph_t pgraph_[2] = {};
  hipGraphExec_t pexec_[2] = {};
  int64_t pcaptured_[2] = {-1, -1};
  hipGraph_t pipe_graph_ = nullptr;
  hipGraphNode_t pipe_root_ = nullptr;
  hipGraphExec_t pipe_exec_ = nullptr;
  int64_t pipe_iters_ = -1;
  const Plan* pipe_next_ = nullptr;
  bool debug_ = false;
  bool check_ = false;
  bool capturing_ = false;
};

}  // namespace jr
