// rocprofiler-sdk interception tool: loaded into target HIP processes via
// ROCP_TOOL_LIBRARIES (or LD_PRELOAD). The MI355X-native replacement for
// the reference's CUPTI producer + eBPF USDT shim:
//
//   - kernel-dispatch buffer tracing   -> KernelDispatchEvent  (timings)
//   - code-object load callbacks       -> CodeObjectLoadEvent  (gfx950 ELF,
//     the cubin-loaded analog, reference parcagpu.go:231-277)
//   - kernel-symbol registration       -> KernelSymbolEvent
//   - gfx950 PC sampling (host-trap or stochastic) -> PCSampleBatch
//   - HIP kernel-launch host stacks    -> LaunchStackEvent (replaces the
//     reference's cudaLaunchKernel uprobe, SURVEY.md §3.3 flow A)
//   - GpuConfig with ns-per-sample     -> GpuConfigEvent (reference
//     GpuConfig.NsPerSample semantics, parca_reporter.go:89-102)
//
// All events flow through a per-process shared-memory ring (ring.h) that
// the agent drains; full-ring drops are counted producer-side.
//
// Configuration via environment:
//   PARCA_GPU_SHM_DIR       ring directory (default /dev/shm)
//   PARCA_GPU_RING_BYTES    ring capacity, power of two (default 32 MiB)
//   PARCA_GPU_PC_SAMPLING   0 disables PC sampling (default on)
//   PARCA_GPU_PC_INTERVAL   host-trap microseconds / stochastic cycles
//   PARCA_GPU_PC_METHOD     "host_trap" (default) or "stochastic"
//   PARCA_GPU_LAUNCH_STACKS 0 disables host launch-stack capture

#include <sys/prctl.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include <execinfo.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include <rocprofiler-sdk/agent.h>
#include <rocprofiler-sdk/buffer.h>
#include <rocprofiler-sdk/buffer_tracing.h>
#include <rocprofiler-sdk/callback_tracing.h>
#include <rocprofiler-sdk/fwd.h>
#include <rocprofiler-sdk/hip/runtime_api_id.h>
#include <rocprofiler-sdk/pc_sampling.h>
#include <rocprofiler-sdk/registration.h>
#include <rocprofiler-sdk/rocprofiler.h>

#include "rocprof/ring.h"

namespace {

using namespace parca;

struct AgentInfo {
  rocprofiler_agent_id_t id;
  uint32_t gpu_index = 0;  // logical GPU index (logical_node_type_id)
  bool pc_configured = false;
  double ns_per_sample = 0.0;
};

struct ToolState {
  rocprofiler_context_id_t ctx{};
  std::vector<rocprofiler_buffer_id_t> buffers;
  std::mutex ring_mu;
  RingProducer* ring = nullptr;
  void* ring_mem = nullptr;
  size_t ring_total = 0;
  std::unordered_map<uint64_t, AgentInfo> agents;  // by agent handle
  bool launch_stacks = true;
  std::atomic<uint64_t> launch_count{0};
  bool initialized = false;
  std::atomic<bool> flusher_run{false};
  std::thread flusher;
  uint64_t duty_on_ms = 0;
  uint64_t duty_off_ms = 0;
};

ToolState* g_state = nullptr;

uint64_t env_u64(const char* name, uint64_t dflt) {
  const char* v = getenv(name);
  if (!v || !*v) return dflt;
  return strtoull(v, nullptr, 0);
}

bool env_flag(const char* name, bool dflt) {
  const char* v = getenv(name);
  if (!v || !*v) return dflt;
  return !(v[0] == '0' || v[0] == 'f' || v[0] == 'F' || v[0] == 'n');
}

void ring_write(uint32_t type, const void* a, size_t na,
                const void* b = nullptr, size_t nb = 0) {
  if (!g_state || !g_state->ring) return;
  std::lock_guard<std::mutex> lk(g_state->ring_mu);
  g_state->ring->write(type, a, na, b, nb);
}

void emit_error(uint32_t code, const char* msg) {
  ErrorEvent ev{code, static_cast<uint32_t>(strlen(msg))};
  ring_write(kEvError, &ev, sizeof(ev), msg, ev.msg_len);
}

bool open_ring() {
  const char* dir = getenv("PARCA_GPU_SHM_DIR");
  if (!dir || !*dir) dir = "/dev/shm";
  // 32 MiB: ~17 s of headroom at a measured launch-storm rate of
  // ~19k events/s (soak evidence). The agent drains every 100 ms but
  // shares a GIL with the CPU-sample pipeline, whose 10 s report flush
  // can starve the drain thread for seconds — bursts must park here.
  // (8 MiB still dropped 2.2% under the 240 s launch-storm soak.)
  uint64_t cap = env_u64("PARCA_GPU_RING_BYTES", 32ull << 20);
  // round up to power of two
  if (cap & (cap - 1)) {
    uint64_t p = 1;
    while (p < cap) p <<= 1;
    cap = p;
  }
  char path[512];
  snprintf(path, sizeof(path), "%s/parca_gpu_%d.ring", dir, getpid());
  int fd = open(path, O_CREAT | O_RDWR, 0600);
  if (fd < 0) return false;
  size_t total = sizeof(RingHeader) + cap;
  if (ftruncate(fd, total) != 0) {
    close(fd);
    return false;
  }
  void* mem = mmap(nullptr, total, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
  close(fd);
  if (mem == MAP_FAILED) return false;
  g_state->ring_mem = mem;
  g_state->ring_total = total;
  g_state->ring = new RingProducer(mem, cap, getpid());
  return true;
}

// -- code object + kernel symbol callbacks --------------------------------

void code_object_cb(rocprofiler_callback_tracing_record_t record,
                    rocprofiler_user_data_t* /*user_data*/,
                    void* /*cb_data*/) {
  if (record.kind != ROCPROFILER_CALLBACK_TRACING_CODE_OBJECT) return;
  if (record.operation == ROCPROFILER_CODE_OBJECT_LOAD) {
    auto* data = static_cast<
        rocprofiler_callback_tracing_code_object_load_data_t*>(record.payload);
    if (record.phase == ROCPROFILER_CALLBACK_PHASE_LOAD) {
      CodeObjectLoadEvent ev{};
      ev.code_object_id = data->code_object_id;
      ev.load_base = data->load_base;
      ev.load_size = data->load_size;
      ev.load_delta = data->load_delta;
      ev.storage_type = static_cast<uint32_t>(data->storage_type);
      if (data->storage_type == ROCPROFILER_CODE_OBJECT_STORAGE_TYPE_MEMORY) {
        ev.memory_base = data->memory_base;
        ev.memory_size = data->memory_size;
      }
      const char* uri = data->uri ? data->uri : "";
      ev.uri_len = static_cast<uint32_t>(strlen(uri));
      if (ev.uri_len > 4096) ev.uri_len = 4096;
      ring_write(kEvCodeObjectLoad, &ev, sizeof(ev), uri, ev.uri_len);
    } else {  // unload
      CodeObjectUnloadEvent ev{data->code_object_id};
      ring_write(kEvCodeObjectUnload, &ev, sizeof(ev));
    }
  } else if (record.operation ==
                 ROCPROFILER_CODE_OBJECT_DEVICE_KERNEL_SYMBOL_REGISTER &&
             record.phase == ROCPROFILER_CALLBACK_PHASE_LOAD) {
    auto* data = static_cast<
        rocprofiler_callback_tracing_code_object_kernel_symbol_register_data_t*>(
        record.payload);
    KernelSymbolEvent ev{};
    ev.kernel_id = data->kernel_id;
    ev.code_object_id = data->code_object_id;
    ev.kernel_object = data->kernel_object;
    const char* name = data->kernel_name ? data->kernel_name : "";
    ev.name_len = static_cast<uint32_t>(strlen(name));
    if (ev.name_len > 1024) ev.name_len = 1024;
    ring_write(kEvKernelSymbol, &ev, sizeof(ev), name, ev.name_len);
  }
}

// -- HIP launch-stack capture ---------------------------------------------

// Launch-stack capture is RATE-LIMITED: glibc backtrace() walks
// .eh_frame and costs ~50-100 us inside libtorch-sized binaries, which
// at eager-mode launch rates (~10k/s) would multiply step time. A token
// bucket caps capture at PARCA_GPU_STACK_RATE stacks/s (default 1000):
// launch-site attribution becomes *sampled*, which is exactly the
// statistical contract of a sampling profiler, while dispatch timing
// stays exact for every kernel. Uncaptured launches are emitted by the
// agent as kernel-only immediately (ring FIFO order guarantees a
// captured stack always precedes its dispatch-completion record).
struct StackBucket {
  std::atomic<int64_t> tokens{0};
  std::atomic<uint64_t> last_refill_s{0};
  int64_t rate = 1000;
};
StackBucket g_stack_bucket;

bool stack_token() {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC_COARSE, &ts);
  uint64_t now = static_cast<uint64_t>(ts.tv_sec);
  uint64_t last = g_stack_bucket.last_refill_s.load(std::memory_order_relaxed);
  if (now != last &&
      g_stack_bucket.last_refill_s.compare_exchange_strong(last, now)) {
    g_stack_bucket.tokens.store(g_stack_bucket.rate,
                                std::memory_order_relaxed);
  }
  return g_stack_bucket.tokens.fetch_sub(1, std::memory_order_relaxed) > 0;
}

void hip_api_cb(rocprofiler_callback_tracing_record_t record,
                rocprofiler_user_data_t* /*user_data*/, void* /*cb_data*/) {
  if (record.phase != ROCPROFILER_CALLBACK_PHASE_ENTER) return;
  if (!stack_token()) return;
  // glibc backtrace: walks .eh_frame, async-signal unsafe but we are in a
  // plain API wrapper here. Depth capped; the first 2-3 frames are
  // rocprofiler + this tool and are trimmed agent-side by mapping.
  void* frames[48];
  int n = backtrace(frames, 48);
  if (n <= 0) return;
  LaunchStackEvent ev{};
  ev.correlation_id = record.correlation_id.internal;
  ev.tid = record.thread_id;
  ev.pid = static_cast<uint32_t>(getpid());
  ev.n_frames = static_cast<uint32_t>(n);
  static_assert(sizeof(void*) == 8, "64-bit only");
  ring_write(kEvLaunchStack, &ev, sizeof(ev), frames, n * sizeof(uint64_t));
  g_state->launch_count.fetch_add(1, std::memory_order_relaxed);
}

// -- kernel dispatch buffer -----------------------------------------------

void dispatch_buffer_cb(rocprofiler_context_id_t /*ctx*/,
                        rocprofiler_buffer_id_t /*buf*/,
                        rocprofiler_record_header_t** headers,
                        size_t num_headers, void* /*data*/,
                        uint64_t drop_count) {
  if (drop_count > 0) emit_error(1, "rocprofiler dispatch buffer dropped");
  for (size_t i = 0; i < num_headers; ++i) {
    auto* h = headers[i];
    if (h == nullptr || h->category != ROCPROFILER_BUFFER_CATEGORY_TRACING ||
        h->kind != ROCPROFILER_BUFFER_TRACING_KERNEL_DISPATCH)
      continue;
    auto* rec =
        static_cast<rocprofiler_buffer_tracing_kernel_dispatch_record_t*>(
            h->payload);
    KernelDispatchEvent ev{};
    ev.correlation_id = rec->correlation_id.internal;
    ev.dispatch_id = rec->dispatch_info.dispatch_id;
    ev.kernel_id = rec->dispatch_info.kernel_id;
    ev.start_ns = rec->start_timestamp;
    ev.end_ns = rec->end_timestamp;
    ev.tid = rec->thread_id;
    ev.pid = static_cast<uint32_t>(getpid());
    auto it = g_state->agents.find(rec->dispatch_info.agent_id.handle);
    ev.gpu_index = it != g_state->agents.end() ? it->second.gpu_index : 0;
    ev.grid[0] = rec->dispatch_info.grid_size.x;
    ev.grid[1] = rec->dispatch_info.grid_size.y;
    ev.grid[2] = rec->dispatch_info.grid_size.z;
    ev.workgroup[0] = rec->dispatch_info.workgroup_size.x;
    ev.workgroup[1] = rec->dispatch_info.workgroup_size.y;
    ev.workgroup[2] = rec->dispatch_info.workgroup_size.z;
    ev.private_segment_size = rec->dispatch_info.private_segment_size;
    ev.group_segment_size = rec->dispatch_info.group_segment_size;
    ring_write(kEvKernelDispatch, &ev, sizeof(ev));
  }
}

// -- PC sampling ----------------------------------------------------------

void pc_sampling_buffer_cb(rocprofiler_context_id_t /*ctx*/,
                           rocprofiler_buffer_id_t /*buf*/,
                           rocprofiler_record_header_t** headers,
                           size_t num_headers, void* data,
                           uint64_t drop_count) {
  if (drop_count > 0) emit_error(2, "rocprofiler pc-sample buffer dropped");
  uint32_t gpu_index = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(data));
  // Batch samples into chunks so one shm record stays bounded.
  constexpr size_t kChunk = 512;
  std::vector<PCSample> chunk;
  chunk.reserve(kChunk < num_headers ? kChunk : num_headers);
  auto flush_chunk = [&]() {
    if (chunk.empty()) return;
    PCSampleBatchHeader bh{gpu_index, static_cast<uint32_t>(chunk.size())};
    ring_write(kEvPCSampleBatch, &bh, sizeof(bh), chunk.data(),
               chunk.size() * sizeof(PCSample));
    chunk.clear();
  };
  for (size_t i = 0; i < num_headers; ++i) {
    auto* h = headers[i];
    if (h == nullptr || h->category != ROCPROFILER_BUFFER_CATEGORY_PC_SAMPLING)
      continue;
    PCSample s{};
    if (h->kind == ROCPROFILER_PC_SAMPLING_RECORD_HOST_TRAP_V0_SAMPLE) {
      auto* r = static_cast<rocprofiler_pc_sampling_record_host_trap_v0_t*>(
          h->payload);
      s.code_object_id = r->pc.code_object_id;
      s.code_object_offset = r->pc.code_object_offset;
      s.timestamp = r->timestamp;
      s.exec_mask = r->exec_mask;
      s.dispatch_id = r->dispatch_id;
      s.correlation_id = r->correlation_id.internal;
      memcpy(&s.hw_id, &r->hw_id, sizeof(uint64_t));
      s.wave_in_group = r->wave_in_group;
      s.flags = 0;
    } else if (h->kind == ROCPROFILER_PC_SAMPLING_RECORD_STOCHASTIC_V0_SAMPLE) {
      auto* r = static_cast<rocprofiler_pc_sampling_record_stochastic_v0_t*>(
          h->payload);
      s.code_object_id = r->pc.code_object_id;
      s.code_object_offset = r->pc.code_object_offset;
      s.timestamp = r->timestamp;
      s.exec_mask = r->exec_mask;
      s.dispatch_id = r->dispatch_id;
      s.correlation_id = r->correlation_id.internal;
      memcpy(&s.hw_id, &r->hw_id, sizeof(uint64_t));
      s.wave_in_group = r->wave_in_group;
      s.flags = pack_pc_flags(/*stochastic=*/true, /*valid=*/true,
                              r->wave_issued != 0, r->inst_type,
                              r->snapshot.reason_not_issued);
    } else {
      continue;  // invalid-sample records are dropped silently
    }
    chunk.push_back(s);
    if (chunk.size() >= kChunk) flush_chunk();
  }
  flush_chunk();
}

rocprofiler_status_t agent_enum_cb(rocprofiler_agent_version_t version,
                                   const void** agents, size_t num_agents,
                                   void* /*user_data*/) {
  if (version != ROCPROFILER_AGENT_INFO_VERSION_0)
    return ROCPROFILER_STATUS_ERROR;
  auto* arr = reinterpret_cast<const rocprofiler_agent_t**>(agents);
  for (size_t i = 0; i < num_agents; ++i) {
    if (arr[i]->type != ROCPROFILER_AGENT_TYPE_GPU) continue;
    AgentInfo info;
    info.id = arr[i]->id;
    info.gpu_index = static_cast<uint32_t>(
        arr[i]->logical_node_type_id >= 0 ? arr[i]->logical_node_type_id : 0);
    g_state->agents.emplace(arr[i]->id.handle, info);
  }
  return ROCPROFILER_STATUS_SUCCESS;
}

void configure_pc_sampling() {
  if (!env_flag("PARCA_GPU_PC_SAMPLING", true)) return;
  const char* method_env = getenv("PARCA_GPU_PC_METHOD");
  bool want_stochastic = method_env && strcmp(method_env, "stochastic") == 0;

  for (auto& [handle, agent] : g_state->agents) {
    // Query what this agent supports right now (another process may
    // already hold a configuration; adopt its interval then).
    std::vector<rocprofiler_pc_sampling_configuration_t> configs;
    auto cb = [](const rocprofiler_pc_sampling_configuration_t* cfgs,
                 size_t n, void* ud) {
      auto* out =
          static_cast<std::vector<rocprofiler_pc_sampling_configuration_t>*>(
              ud);
      out->assign(cfgs, cfgs + n);
      return ROCPROFILER_STATUS_SUCCESS;
    };
    if (rocprofiler_query_pc_sampling_agent_configurations(
            agent.id, cb, &configs) != ROCPROFILER_STATUS_SUCCESS ||
        configs.empty())
      continue;

    const rocprofiler_pc_sampling_configuration_t* picked = nullptr;
    for (auto& c : configs) {
      if (want_stochastic &&
          c.method == ROCPROFILER_PC_SAMPLING_METHOD_STOCHASTIC) {
        picked = &c;
        break;
      }
      if (!want_stochastic &&
          c.method == ROCPROFILER_PC_SAMPLING_METHOD_HOST_TRAP) {
        picked = &c;
        break;
      }
    }
    if (!picked) picked = &configs.front();

    uint64_t interval;
    if (picked->min_interval == picked->max_interval) {
      interval = picked->min_interval;  // adopted from another process
    } else {
      uint64_t dflt = picked->method == ROCPROFILER_PC_SAMPLING_METHOD_HOST_TRAP
                          ? 10000        // 10 ms host-trap
                          : (1u << 20);  // 2^20 cycles stochastic
      interval = env_u64("PARCA_GPU_PC_INTERVAL", dflt);
      if (interval < picked->min_interval) interval = picked->min_interval;
      if (interval > picked->max_interval) interval = picked->max_interval;
      if (picked->flags &
          ROCPROFILER_PC_SAMPLING_CONFIGURATION_FLAGS_INTERVAL_POW2) {
        uint64_t p = 1;
        while ((p << 1) <= interval) p <<= 1;
        interval = p;
      }
    }

    rocprofiler_buffer_id_t buffer_id{};
    if (rocprofiler_create_buffer(
            g_state->ctx, 4 << 20, 2 << 20, ROCPROFILER_BUFFER_POLICY_LOSSLESS,
            pc_sampling_buffer_cb,
            reinterpret_cast<void*>(static_cast<uintptr_t>(agent.gpu_index)),
            &buffer_id) != ROCPROFILER_STATUS_SUCCESS)
      continue;

    auto status = rocprofiler_configure_pc_sampling_service(
        g_state->ctx, agent.id, picked->method, picked->unit, interval,
        buffer_id, 0);
    if (status != ROCPROFILER_STATUS_SUCCESS) {
      emit_error(3, rocprofiler_get_status_string(status));
      rocprofiler_destroy_buffer(buffer_id);
      continue;
    }
    g_state->buffers.push_back(buffer_id);
    rocprofiler_callback_thread_t thr{};
    if (rocprofiler_create_callback_thread(&thr) ==
        ROCPROFILER_STATUS_SUCCESS)
      rocprofiler_assign_callback_thread(buffer_id, thr);

    agent.pc_configured = true;
    // ns per sample for the gpu_pcsample/count period
    // (GpuConfig.NsPerSample analog).
    double nsps = 0.0;
    if (picked->unit == ROCPROFILER_PC_SAMPLING_UNIT_TIME) {
      nsps = static_cast<double>(interval) * 1e3;  // micro -> nanoseconds
    } else if (picked->unit == ROCPROFILER_PC_SAMPLING_UNIT_CYCLES) {
      // gfx950 max clock 2.4 GHz; actual clock varies — report nominal.
      nsps = static_cast<double>(interval) / 2.4;
    }
    agent.ns_per_sample = nsps;
    GpuConfigEvent ev{};
    ev.gpu_index = agent.gpu_index;
    ev.method = static_cast<uint32_t>(picked->method);
    ev.unit = static_cast<uint32_t>(picked->unit);
    ev.interval = interval;
    ev.ns_per_sample = nsps;
    ring_write(kEvGpuConfig, &ev, sizeof(ev));
  }
}

int tool_init(rocprofiler_client_finalize_t /*fini*/, void* /*tool_data*/) {
  if (!open_ring()) {
    fprintf(stderr, "[parca-rocprof] failed to open shm ring; disabled\n");
    return -1;
  }
  rocprofiler_query_available_agents(ROCPROFILER_AGENT_INFO_VERSION_0,
                                     agent_enum_cb,
                                     sizeof(rocprofiler_agent_t), nullptr);
  if (rocprofiler_create_context(&g_state->ctx) !=
      ROCPROFILER_STATUS_SUCCESS)
    return -1;

  // Code objects + kernel symbols.
  rocprofiler_configure_callback_tracing_service(
      g_state->ctx, ROCPROFILER_CALLBACK_TRACING_CODE_OBJECT, nullptr, 0,
      code_object_cb, nullptr);

  // Kernel dispatch timing through a buffered service.
  rocprofiler_buffer_id_t dispatch_buf{};
  if (rocprofiler_create_buffer(g_state->ctx, 1 << 20, 512 << 10,
                                ROCPROFILER_BUFFER_POLICY_LOSSLESS,
                                dispatch_buffer_cb, nullptr,
                                &dispatch_buf) == ROCPROFILER_STATUS_SUCCESS) {
    rocprofiler_configure_buffer_tracing_service(
        g_state->ctx, ROCPROFILER_BUFFER_TRACING_KERNEL_DISPATCH, nullptr, 0,
        dispatch_buf);
    g_state->buffers.push_back(dispatch_buf);
    rocprofiler_callback_thread_t thr{};
    if (rocprofiler_create_callback_thread(&thr) ==
        ROCPROFILER_STATUS_SUCCESS)
      rocprofiler_assign_callback_thread(dispatch_buf, thr);
  }

  // Host launch stacks for the GPU<->CPU joined flamegraph.
  g_state->launch_stacks = env_flag("PARCA_GPU_LAUNCH_STACKS", true);
  g_stack_bucket.rate =
      static_cast<int64_t>(env_u64("PARCA_GPU_STACK_RATE", 1000));
  if (g_state->launch_stacks) {
    static const rocprofiler_tracing_operation_t launch_ops[] = {
        ROCPROFILER_HIP_RUNTIME_API_ID_hipLaunchKernel,
        ROCPROFILER_HIP_RUNTIME_API_ID_hipExtLaunchKernel,
        ROCPROFILER_HIP_RUNTIME_API_ID_hipModuleLaunchKernel,
        ROCPROFILER_HIP_RUNTIME_API_ID_hipExtModuleLaunchKernel,
        ROCPROFILER_HIP_RUNTIME_API_ID_hipLaunchCooperativeKernel,
        ROCPROFILER_HIP_RUNTIME_API_ID_hipGraphLaunch,
    };
    rocprofiler_configure_callback_tracing_service(
        g_state->ctx, ROCPROFILER_CALLBACK_TRACING_HIP_RUNTIME_API,
        launch_ops, sizeof(launch_ops) / sizeof(launch_ops[0]), hip_api_cb,
        nullptr);
    // Warm up glibc backtrace (first call dlopens libgcc).
    void* warm[4];
    backtrace(warm, 4);
  }

  configure_pc_sampling();

  int valid = 0;
  rocprofiler_context_is_valid(g_state->ctx, &valid);
  if (valid == 0) return -1;
  // PARCA_GPU_DEFER_START=1 leaves the context stopped; the host process
  // (e.g. bench.py measuring a clean baseline phase) starts it later via
  // the exported parca_rocprof_start().
  if (!env_flag("PARCA_GPU_DEFER_START", false)) {
    if (rocprofiler_start_context(g_state->ctx) != ROCPROFILER_STATUS_SUCCESS)
      return -1;
  }
  g_state->initialized = true;

  // Optional duty-cycling: PARCA_GPU_DUTY_CYCLE="on_ms,off_ms" toggles
  // the tracing context so the dispatch-intercept cost scales by
  // on/(on+off). Kernel timing becomes duty-cycled *sampling*; the agent
  // rescales values by the advertised factor (GpuConfig method 100) so
  // pprof totals stay statistically correct.
  uint64_t duty_on_ms = 0, duty_off_ms = 0;
  if (const char* duty = getenv("PARCA_GPU_DUTY_CYCLE");
      duty && *duty) {
    if (sscanf(duty, "%lu,%lu", &duty_on_ms, &duty_off_ms) != 2 ||
        duty_on_ms == 0)
      duty_on_ms = duty_off_ms = 0;
  }
  if (duty_on_ms > 0 && duty_off_ms > 0) {
    GpuConfigEvent ev{};
    ev.gpu_index = 0;
    ev.method = 100;  // duty-cycle advertisement
    ev.unit = 0;
    ev.interval = duty_on_ms;
    ev.ns_per_sample =
        static_cast<double>(duty_on_ms + duty_off_ms) / duty_on_ms;
    ring_write(kEvGpuConfig, &ev, sizeof(ev));
  }
  g_state->duty_on_ms = duty_on_ms;
  g_state->duty_off_ms = duty_off_ms;

  // Periodic flush so kernel timings reach the shm ring promptly instead
  // of waiting for the buffer watermark or process exit (the agent needs
  // them within its 10 s report interval). The same thread drives the
  // duty cycle.
  g_state->flusher_run.store(true);
  g_state->flusher = std::thread([]() {
    uint64_t elapsed_ms = 0;
    bool ctx_on = true;
    const uint64_t on_ms = g_state->duty_on_ms;
    const uint64_t off_ms = g_state->duty_off_ms;
    while (g_state->flusher_run.load(std::memory_order_relaxed)) {
      struct timespec ts{0, 100 * 1000 * 1000};
      nanosleep(&ts, nullptr);
      elapsed_ms += 100;
      if (elapsed_ms % 500 == 0)
        for (auto& buf : g_state->buffers) rocprofiler_flush_buffer(buf);
      if (on_ms > 0 && off_ms > 0) {
        if (ctx_on && elapsed_ms >= on_ms) {
          rocprofiler_stop_context(g_state->ctx);
          ctx_on = false;
          elapsed_ms = 0;
        } else if (!ctx_on && elapsed_ms >= off_ms) {
          rocprofiler_start_context(g_state->ctx);
          ctx_on = true;
          elapsed_ms = 0;
        }
      }
    }
    if (!ctx_on) rocprofiler_start_context(g_state->ctx);
  });
  return 0;
}

void tool_fini(void* /*tool_data*/) {
  if (!g_state) return;
  g_state->flusher_run.store(false);
  if (g_state->flusher.joinable()) g_state->flusher.join();
  for (auto& buf : g_state->buffers) rocprofiler_flush_buffer(buf);
  // Leave the ring mapped; the kernel reclaims at process exit and the
  // agent unlinks the file once the pid is gone.
}

}  // namespace

// Runtime control for host processes that dlopen this library (it is
// already loaded in-process via ROCP_TOOL_LIBRARIES, so dlopen returns
// the same handle): start/stop the tracing context around measurement
// phases, and report producer-side stats.
extern "C" int parca_rocprof_start() {
  if (!g_state || !g_state->initialized) return -1;
  return rocprofiler_start_context(g_state->ctx) == ROCPROFILER_STATUS_SUCCESS
             ? 0
             : -2;
}

extern "C" int parca_rocprof_stop() {
  if (!g_state || !g_state->initialized) return -1;
  for (auto& buf : g_state->buffers) rocprofiler_flush_buffer(buf);
  return rocprofiler_stop_context(g_state->ctx) == ROCPROFILER_STATUS_SUCCESS
             ? 0
             : -2;
}

extern "C" int parca_rocprof_flush() {
  if (!g_state || !g_state->initialized) return -1;
  for (auto& buf : g_state->buffers) rocprofiler_flush_buffer(buf);
  return 0;
}

// stats[0]=ring written, stats[1]=ring dropped, stats[2]=launch stacks
extern "C" int parca_rocprof_stats(uint64_t* stats) {
  if (!g_state || !g_state->ring) return -1;
  stats[0] = g_state->ring->header()->written.load();
  stats[1] = g_state->ring->header()->dropped.load();
  stats[2] = g_state->launch_count.load();
  return 0;
}

extern "C" rocprofiler_tool_configure_result_t* rocprofiler_configure(
    uint32_t version, const char* runtime_version, uint32_t priority,
    rocprofiler_client_id_t* id) {
  (void)version;
  (void)runtime_version;
  (void)priority;
  id->name = "parca-agent-amd";
  // Let the (non-ancestor) agent daemon read this process's memory on
  // Yama ptrace_scope=1 systems without CAP_SYS_PTRACE: interpreter
  // unwinding and memory:// code-object fetches use process_vm_readv,
  // which Yama subjects to the ptrace ancestry check. The injected
  // profiler tool opting its host in is the sanctioned mechanism
  // (PR_SET_PTRACER_ANY); processes without the tool need the agent to
  // hold CAP_SYS_PTRACE (deploy/parca-agent-amd.yaml grants it).
#ifdef PR_SET_PTRACER
  prctl(PR_SET_PTRACER, PR_SET_PTRACER_ANY, 0, 0, 0);
#endif
  g_state = new ToolState();
  static rocprofiler_tool_configure_result_t cfg{
      sizeof(rocprofiler_tool_configure_result_t), &tool_init, &tool_fini,
      nullptr};
  return &cfg;
}
