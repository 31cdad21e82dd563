// ocean_capi_exchange.cpp — the part of the C ABI (include/oceanfft.h) that moves a slab frame's blocks
// between the ranks: the RCCL communicator and ocean_generator_slab_frame[_pipelined], and the one-sided
// exchange (ocean_peers) with the *_put* entry points. The passes they drive are the generator unit's
// (ocean_capi.cpp), declared in ocean_capi_internal.h.
#include "oceanfft.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "ocean_capi_internal.h"
#include "ocean_internal.h"

// ---------------------------------------------------------------------------------------------
// Slab exchange over RCCL: the equal-split all-to-all between the column and the row pass (SURVEY
// §8e), as P grouped ncclSend / ncclRecv pairs of exchange_bytes / P on the generator's streams.
// ---------------------------------------------------------------------------------------------
struct ocean_comm
{
  ncclComm_t comm = nullptr;
  int nranks = 0, rank = 0;
  bool owned = false;
};

namespace
{
int nccl_fail(ncclResult_t r, const char* what)
{
  return fail(OCEAN_ERR_HIP, std::string(what) + ": " + ncclGetErrorString(r));
}

// The equal-split all-to-all of blk bytes per rank pair, enqueued on `stream`: one group of
// ncclSend / ncclRecv pairs, each block in pieces of at most kExchangePiece bytes (RCCL 2.26 corrupted
// a single send / receive above 1 GiB in a world-size-1 self exchange: tools/rccl_selfcheck.py,
// profiles/r03_rccl_selfcheck.log; a whole 8192^2 block is 1.35 GB).
constexpr size_t kExchangePiece = (size_t)512 << 20;

int exchange_bytes_all_to_all(ocean_comm* c, const unsigned char* send, unsigned char* recv, size_t blk,
                              hipStream_t stream)
{
  ncclResult_t r = ncclGroupStart();
  for (int q = 0; q < c->nranks && r == ncclSuccess; q++)
    for (size_t o = 0; o < blk && r == ncclSuccess; o += kExchangePiece)
    {
      const size_t len = std::min(kExchangePiece, blk - o);
      r = ncclSend(send + q * blk + o, len, ncclUint8, q, c->comm, stream);
      if (r == ncclSuccess)
        r = ncclRecv(recv + q * blk + o, len, ncclUint8, q, c->comm, stream);
    }
  const ncclResult_t e = ncclGroupEnd();
  if (r != ncclSuccess)
    return nccl_fail(r, "slab exchange (ncclSend / ncclRecv)");
  if (e != ncclSuccess)
    return nccl_fail(e, "slab exchange (ncclGroupEnd)");
  return OCEAN_OK;
}

// The two exchange slots, the comm stream and its events (first use, or after a path switch that
// changed exchange_bytes).
int frame_slots(ocean_generator* g)
{
  const size_t bytes = ocean_generator_exchange_bytes(g);
  if (g->xslot_bytes < bytes)
  {
    if (g->pending_slot >= 0)
      return fail(OCEAN_ERR_INVALID, "slab frame: the exchange size changed with a frame in flight (flush first)");
    for (int k = 0; k < 2; k++)
      for (unsigned char** p : {&g->xsend[k], &g->xrecv[k]})
      {
        if (*p)
          (void)hipFree(*p);
        *p = nullptr;
      }
    g->xslot_bytes = 0;
    for (int k = 0; k < 2; k++)
    {
      HIP_TRY(hipMalloc(&g->xsend[k], bytes), "slab frame: exchange buffers");
      HIP_TRY(hipMalloc(&g->xrecv[k], bytes), "slab frame: exchange buffers");
    }
    g->xslot_bytes = bytes;
  }
  if (!g->comm_stream)
  {
    HIP_TRY(hipStreamCreateWithFlags(&g->comm_stream, hipStreamNonBlocking), "slab frame: comm stream");
    for (int k = 0; k < 2; k++)
      for (hipEvent_t* ev : {&g->cols_done[k], &g->xchg_done[k], &g->rows_done[k]})
        HIP_TRY(hipEventCreateWithFlags(ev, hipEventDisableTiming), "slab frame: events");
  }
  return OCEAN_OK;
}

int check_comm(const ocean_generator* g, const ocean_comm* c, const char* who)
{
  if (!g || !c || !c->comm)
    return fail(OCEAN_ERR_INVALID, std::string(who) + ": null generator or communicator");
  if (c->nranks != g->ranks || c->rank != g->rank)
    return fail(OCEAN_ERR_INVALID, std::string(who) + ": communicator rank " + std::to_string(c->rank) + " of " +
                                       std::to_string(c->nranks) + " does not match slab rank " +
                                       std::to_string(g->rank) + " of " + std::to_string(g->ranks));
  return OCEAN_OK;
}

// Row pass of the frame in slot s (its own column-pass values: pipelined rows run after the next
// frame's column pass).
int slot_rows(ocean_generator* g, int s)
{
  ocean_fft* f = g->fft;
  HIP_TRY(hipStreamWaitEvent(f->stream, g->xchg_done[s], 0), "slab frame: wait for the exchange");
  TRY(generator_rows(g, reinterpret_cast<const float4*>(g->xrecv[s]), g->slot_state[s]));
  HIP_TRY(hipEventRecord(g->rows_done[s], f->stream), "slab frame: events");
  g->rows_recorded[s] = true;
  return OCEAN_OK;
}

// Column pass of frame f into slot f % 2 and its exchange (send slot -> recv slot) on the comm stream.
int slot_columns_and_exchange(ocean_generator* g, ocean_comm* c, float timestep, int update_spectrum, int& slot)
{
  ocean_fft* f = g->fft;
  const int s = (int)(g->frames_issued % 2);
  TRY(generator_columns(g, timestep, update_spectrum, reinterpret_cast<float4*>(g->xsend[s])));
  g->slot_state[s] = current_frame(g);
  HIP_TRY(hipEventRecord(g->cols_done[s], f->stream), "slab frame: events");
  HIP_TRY(hipStreamWaitEvent(g->comm_stream, g->cols_done[s], 0), "slab frame: stream order");
  if (g->rows_recorded[s])  // frame f - 2's row pass has finished reading recv[s]
    HIP_TRY(hipStreamWaitEvent(g->comm_stream, g->rows_done[s], 0), "slab frame: stream order");
  TRY(exchange_bytes_all_to_all(c, g->xsend[s], g->xrecv[s], ocean_generator_exchange_bytes(g) / g->ranks,
                                g->comm_stream));
  HIP_TRY(hipEventRecord(g->xchg_done[s], g->comm_stream), "slab frame: events");
  g->frames_issued++;
  slot = s;
  return OCEAN_OK;
}
}  // namespace

extern "C" {

int ocean_comm_unique_id(unsigned char id[OCEAN_COMM_ID_BYTES])
{
  static_assert(OCEAN_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "RCCL unique id size");
  if (!id)
    return fail(OCEAN_ERR_INVALID, "ocean_comm_unique_id: null id");
  ncclUniqueId u;
  const ncclResult_t r = ncclGetUniqueId(&u);
  if (r != ncclSuccess)
    return nccl_fail(r, "ncclGetUniqueId");
  std::memcpy(id, u.internal, NCCL_UNIQUE_ID_BYTES);
  return OCEAN_OK;
}

int ocean_comm_create(ocean_comm** out, const unsigned char id[OCEAN_COMM_ID_BYTES], int nranks, int rank)
{
  if (!out || !id || nranks < 1 || rank < 0 || rank >= nranks)
    return fail(OCEAN_ERR_INVALID, "ocean_comm_create: null argument or rank outside [0, nranks)");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(OCEAN_ERR_NO_DEVICE, "ocean_comm_create: no HIP device visible");
  ncclUniqueId u;
  std::memcpy(u.internal, id, NCCL_UNIQUE_ID_BYTES);
  auto* c = new ocean_comm();
  const ncclResult_t r = ncclCommInitRank(&c->comm, nranks, u, rank);
  if (r != ncclSuccess)
  {
    delete c;
    return nccl_fail(r, "ncclCommInitRank");
  }
  c->nranks = nranks;
  c->rank = rank;
  c->owned = true;
  *out = c;
  return OCEAN_OK;
}

int ocean_comm_wrap(ocean_comm** out, void* nccl_comm, int nranks, int rank)
{
  if (!out || !nccl_comm || nranks < 1 || rank < 0 || rank >= nranks)
    return fail(OCEAN_ERR_INVALID, "ocean_comm_wrap: null argument or rank outside [0, nranks)");
  *out = nullptr;
  // the exchange addresses peers by these values: they must be the communicator's own
  const ncclComm_t nc = static_cast<ncclComm_t>(nccl_comm);
  int count = 0, user_rank = 0;
  ncclResult_t r = ncclCommCount(nc, &count);
  if (r == ncclSuccess)
    r = ncclCommUserRank(nc, &user_rank);
  if (r != ncclSuccess)
    return nccl_fail(r, "ocean_comm_wrap: ncclCommCount / ncclCommUserRank");
  if (count != nranks || user_rank != rank)
    return fail(OCEAN_ERR_INVALID, "ocean_comm_wrap: the communicator is rank " + std::to_string(user_rank) + " of " +
                                       std::to_string(count) + ", not rank " + std::to_string(rank) + " of " +
                                       std::to_string(nranks));
  auto* c = new ocean_comm();
  c->comm = nc;
  c->nranks = nranks;
  c->rank = rank;
  *out = c;
  return OCEAN_OK;
}

int ocean_comm_destroy(ocean_comm* comm)
{
  if (!comm)
    return OCEAN_OK;
  ncclResult_t r = ncclSuccess;
  if (comm->owned && comm->comm)
    r = ncclCommDestroy(comm->comm);
  delete comm;
  return r == ncclSuccess ? OCEAN_OK : nccl_fail(r, "ncclCommDestroy");
}

int ocean_comm_all_to_all(ocean_comm* comm, const void* send, void* recv, size_t bytes, void* hip_stream)
{
  if (!comm || !comm->comm || (bytes > 0 && (!send || !recv)) || bytes % comm->nranks != 0)
    return fail(OCEAN_ERR_INVALID, "ocean_comm_all_to_all: null argument or bytes not a multiple of the rank count");
  return exchange_bytes_all_to_all(comm, static_cast<const unsigned char*>(send), static_cast<unsigned char*>(recv),
                                   bytes / comm->nranks, (hipStream_t)hip_stream);
}

int ocean_generator_slab_frame(ocean_generator* g, ocean_comm* comm, float timestep, int update_spectrum)
{
  TRY(check_comm(g, comm, "ocean_generator_slab_frame"));
  TRY(ocean_generator_slab_flush(g));  // a pipelined frame in flight lands first
  TRY(frame_slots(g));
  int s = 0;
  TRY(slot_columns_and_exchange(g, comm, timestep, update_spectrum, s));
  return slot_rows(g, s);
}

int ocean_generator_slab_frame_pipelined(ocean_generator* g, ocean_comm* comm, float timestep, int update_spectrum)
{
  TRY(check_comm(g, comm, "ocean_generator_slab_frame_pipelined"));
  TRY(frame_slots(g));
  int s = 0;
  TRY(slot_columns_and_exchange(g, comm, timestep, update_spectrum, s));
  if (g->pending_slot >= 0)
    TRY(slot_rows(g, g->pending_slot));
  g->pending_slot = s;
  return OCEAN_OK;
}

int ocean_generator_slab_flush(ocean_generator* g)
{
  if (!g)
    return fail(OCEAN_ERR_INVALID, "ocean_generator_slab_flush: null generator");
  if (g->pending_slot < 0)
    return OCEAN_OK;
  const int s = g->pending_slot;
  g->pending_slot = -1;
  return slot_rows(g, s);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// The one-sided slab exchange (ocean_peers): the four-step column pass stores block q into rank q's
// receive slot through a peer mapping, and per-frame flag words replace the all-to-all (SURVEY §8e;
// DESIGN.md §6 "one-sided exchange").
// ---------------------------------------------------------------------------------------------
namespace
{
constexpr int kMaxRanks = 16;
constexpr int kReadyWord = 0, kFreedWord = 16, kReleaseCounter = 40, kErrWord = 48, kFlagWords = 64;
constexpr uint32_t kPeerMagic = 0x4f505231;  // "OPR1"

struct PeerHandle
{
  uint32_t magic;
  int32_t rank, ranks;
  uint32_t flags_uncached;
  uint64_t slot_bytes;
  hipIpcMemHandle_t data, flags;
};
static_assert(sizeof(PeerHandle) <= OCEAN_PEER_HANDLE_BYTES, "peer handle size");
}  // namespace

struct ocean_peers
{
  ocean_generator* g = nullptr;
  int rank = 0, ranks = 1;
  size_t blk = 0, slot = 0;        // block bytes, slot bytes (ranks * blk = the exchange bytes)
  unsigned char* data = nullptr;   // this rank's two receive slots
  uint32_t* flags = nullptr;       // this rank's flag words: ready[16] | freed[16] | .. | release counter @ 40 | err @ 48
  bool flags_uncached = false;
  unsigned char* peer_data[kMaxRanks] = {};
  uint32_t* peer_flags[kMaxRanks] = {};
  bool mapped[2 * kMaxRanks] = {};  // data / flags opened with hipIpcOpenMemHandle (closed on destroy)
  bool connected = false;
  uint64_t* table = nullptr;       // device: put destinations [2 slots][16], then the flag arrays [16]
  // pipelined frames: step 1 on s1_stream into parts slot f % 2, the put on put_stream, the row pass
  // on the generator's stream (ocean_peers_set_streams can replace the first two)
  hipStream_t s1_stream = nullptr, put_stream = nullptr, row_stream = nullptr;
  hipStream_t own_s1 = nullptr, own_put = nullptr, own_rows = nullptr;
  int put_cus_per_xcd = 0;           // own streams CU-masked: the put on this many CUs of every XCD
  int row_cus = 0;                   // the CUs the own row stream may use when masked (0: all)
  int caller_row_cus = 0;            // ocean_peers_set_row_cus: the caller's row stream's CUs (0: all)
  hipEvent_t rows_done = nullptr;    // pipelined rows on row_stream -> the generator's stream
  hipEvent_t gen_ready = nullptr;    // the generator's stream -> pipelined rows (caller work on the maps)
  bool failed = false;               // a wait timed out (ocean_peers_synchronize): frames are refused
  unsigned char* parts2 = nullptr;   // step 1's second parts slot
  hipEvent_t s1_done[2] = {nullptr, nullptr}, put_done[2] = {nullptr, nullptr};
  bool put_done_valid[2] = {false, false};
  long long deadline = 0;          // wall-clock ticks
  int timeout_ms = 20000;
  int put_cus = 0;
  int64_t frames = 0;              // frames whose column pass was issued
  int64_t rows = 0;                // frames whose row pass was issued
  FrameState slot_state[2];        // the frame in each receive slot
};

bool peers_pending(const ocean_peers* p) { return p && p->rows < p->frames; }

void peers_detach(ocean_peers* p)
{
  if (!p)
    return;
  for (hipStream_t st : {p->s1_stream, p->put_stream, p->row_stream})
    if (st)
      (void)hipStreamSynchronize(st);
  p->g = nullptr;
  p->connected = false;
}

namespace
{
int peers_deadline(ocean_peers* p)
{
  int khz = 0;
  HIP_TRY(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, p->g ? p->g->fft->device : 0),
          "ocean_peers: wall clock rate");
  p->deadline = (long long)(khz > 0 ? khz : 100000) * p->timeout_ms;
  return OCEAN_OK;
}

int check_peers(const ocean_generator* g, const ocean_peers* p, const char* who)
{
  if (!g || !p || p->g != g)
    return fail(OCEAN_ERR_INVALID, std::string(who) + ": null generator, or peers created for another generator");
  if (!p->connected)
    return fail(OCEAN_ERR_INVALID, std::string(who) + ": ocean_peers_connect has not run");
  if (p->failed)
    return fail(OCEAN_ERR_TIMEOUT, std::string(who) + ": a one-sided wait timed out earlier (ocean_peers_synchronize "
                                                      "reported it); the ranks' flags are out of step: destroy and "
                                                      "recreate the peers");
  if (!half_slab_path(g) || hslab_xbuf_bytes(g) != p->slot)
    return fail(OCEAN_ERR_INVALID, std::string(who) + ": the generator left the half-spectrum slab path (or its "
                                                      "exchange size changed) since ocean_peers_create");
  return OCEAN_OK;
}

// the device table: dst[s][q] = rank q's slot s + this rank's block offset, then the flag arrays
int peers_table(ocean_peers* p)
{
  uint64_t host[3 * kMaxRanks] = {};
  for (int s = 0; s < 2; s++)
    for (int q = 0; q < p->ranks; q++)
      host[s * kMaxRanks + q] = (uint64_t)(uintptr_t)(p->peer_data[q] + s * p->slot + (size_t)p->rank * p->blk);
  for (int q = 0; q < p->ranks; q++)
    host[2 * kMaxRanks + q] = (uint64_t)(uintptr_t)p->peer_flags[q];
  HIP_TRY(hipMemcpy(p->table, host, sizeof(host), hipMemcpyHostToDevice), "ocean_peers: destination table");
  p->connected = true;
  return OCEAN_OK;
}

PeerWait peer_wait(ocean_peers* p, int word0, int64_t target)
{
  return PeerWait{p->flags, word0, p->ranks, (uint32_t)target, p->deadline, p->flags + kErrWord};
}

uint32_t* const* flag_table(const ocean_peers* p)
{
  return reinterpret_cast<uint32_t* const*>(p->table + 2 * kMaxRanks);
}

// Column pass of frame f = p->frames into every rank's slot f % 2, then this rank's "ready" word (f + 1)
// in every rank's flags. The put waits until every rank has finished reading that slot (frame f - 2's
// row pass). Serial: all on the generator's stream. Pipelined: step 1 on s1_stream into parts slot f % 2
// (after the put of frame f - 2 read that slot), the put on put_stream after step 1, so step 1 of frame
// f + 1 and the row pass of frame f - 1 run beside the put of frame f.
int put_columns(ocean_generator* g, ocean_peers* p, float timestep, int update_spectrum, bool pipelined)
{
  ocean_fft* fs = g->fft;
  const int64_t f = p->frames;
  const int s = (int)(f % 2);
  const PeerWait w = peer_wait(p, kFreedWord, f - 1);
  Gen4Put put{p->table + s * kMaxRanks, f >= 2 ? &w : nullptr, p->put_cus};
  hipStream_t cs = nullptr;
  if (pipelined && frame_path(g) == FramePath::FourStep)
  {
    if (!p->parts2)
      HIP_TRY(hipMalloc(&p->parts2, gen4_parts_bytes(fs->logn, g->cascades, g->g4)), "one-sided exchange: parts slot");
    cs = p->s1_stream;
    put.parts = s ? p->parts2 : g->parts;
    put.stream = p->put_stream;
    put.handoff = p->s1_done[s];
    if (p->put_done_valid[s])
      HIP_TRY(hipStreamWaitEvent(cs, p->put_done[s], 0), "one-sided exchange: parts slot reuse");
  }
  else if (pipelined)
    cs = p->put_stream;  // the strip-dealt pass stores its blocks itself: all of it on the put stream
  else
    for (int k = 0; k < 2; k++)  // a serial frame after pipelined ones: its step 1 rewrites parts slot 0
      if (p->put_done_valid[k])
      {
        HIP_TRY(hipStreamWaitEvent(fs->stream, p->put_done[k], 0), "one-sided exchange: stream order");
        p->put_done_valid[k] = false;
      }
  TRY(generator_columns(g, timestep, update_spectrum, nullptr, &put, cs));
  hipStream_t ps = pipelined ? p->put_stream : fs->stream;
  HIP_TRY(launch_peer_signal_release(flag_table(p), p->ranks, kReadyWord + p->rank, (uint32_t)(f + 1),
                                     p->flags + kReleaseCounter, ps),
          "one-sided exchange: ready signal");
  if (pipelined)
  {
    HIP_TRY(hipEventRecord(p->put_done[s], ps), "one-sided exchange: events");
    p->put_done_valid[s] = true;
  }
  p->slot_state[s] = current_frame(g);
  p->frames = f + 1;
  return OCEAN_OK;
}

// Row pass of the oldest frame whose rows are not issued yet: wait for every rank's blocks, rows, then
// this rank's "freed" word (f + 1) in every rank's flags. Serial: on the generator's stream. Pipelined:
// on the peers' row stream, which the generator's stream then waits for (the maps stay ordered on it).
int put_rows(ocean_generator* g, ocean_peers* p, bool pipelined = false)
{
  ocean_fft* f = g->fft;
  const int64_t fr = p->rows;
  if (fr >= p->frames)
    return fail(OCEAN_ERR_INVALID, "ocean_generator_slab_put_rows: no column pass issued for this frame");
  const int s = (int)(fr % 2);
  hipStream_t rs = pipelined ? p->row_stream : f->stream;
  if (rs != f->stream)
  {
    // the row pass rewrites g->maps / jac: after the caller's work on the generator's stream (the
    // header keeps the maps ordered there)
    HIP_TRY(hipEventRecord(p->gen_ready, f->stream), "one-sided exchange: events");
    HIP_TRY(hipStreamWaitEvent(rs, p->gen_ready, 0), "one-sided exchange: stream order");
  }
  HIP_TRY(launch_peer_wait(peer_wait(p, kReadyWord, fr + 1), rs), "one-sided exchange: ready wait");
  TRY(generator_rows(g, reinterpret_cast<const float4*>(p->data + s * p->slot), p->slot_state[s], rs,
                     rs == p->own_rows ? p->row_cus : p->caller_row_cus));
  HIP_TRY(launch_peer_signal(flag_table(p), p->ranks, kFreedWord + p->rank, (uint32_t)(fr + 1), rs),
          "one-sided exchange: freed signal");
  if (rs != f->stream)
  {
    HIP_TRY(hipEventRecord(p->rows_done, rs), "one-sided exchange: events");
    HIP_TRY(hipStreamWaitEvent(f->stream, p->rows_done, 0), "one-sided exchange: stream order");
  }
  p->rows = fr + 1;
  return OCEAN_OK;
}

// (Re)create the peers' own streams; with put_cus_per_xcd > 0 CU-masked: the put stream on that many
// CUs of every XCD, the step-1 and row streams on the others. A hipExtStreamCreateWithCUMask bit c is
// CU c / 8 of XCD c % 8, and an XCD whose bits are all clear runs on all its CUs (workgroups are dealt
// to every XCD whatever the mask; tools/xcdmask, profiles/r05_xcdprobe.log): a mask can only split
// each XCD, so the put takes the same share of each.
int peers_streams(ocean_peers* p)
{
  for (hipStream_t* st : {&p->own_s1, &p->own_put, &p->own_rows})
    if (*st)
    {
      HIP_TRY(hipStreamSynchronize(*st), "ocean_peers: streams");
      HIP_TRY(hipStreamDestroy(*st), "ocean_peers: streams");
      *st = nullptr;
    }
  const int cus = p->g->fft->device_cus;
  if (p->put_cus_per_xcd > 0 && cus % 8 == 0 && p->put_cus_per_xcd < cus / 8)
  {
    std::vector<uint32_t> put((cus + 31) / 32, 0u), rest((cus + 31) / 32, 0u);
    for (int c = 0; c < cus; c++)
      (c / 8 < p->put_cus_per_xcd ? put : rest)[c / 32] |= 1u << (c % 32);
    HIP_TRY(hipExtStreamCreateWithCUMask(&p->own_put, (uint32_t)put.size(), put.data()), "ocean_peers: put stream");
    HIP_TRY(hipExtStreamCreateWithCUMask(&p->own_s1, (uint32_t)rest.size(), rest.data()), "ocean_peers: column stream");
    HIP_TRY(hipExtStreamCreateWithCUMask(&p->own_rows, (uint32_t)rest.size(), rest.data()), "ocean_peers: row stream");
    p->row_cus = cus - 8 * p->put_cus_per_xcd;  // resident row-pass grids sized to the masked stream
  }
  else
  {
    for (hipStream_t* st : {&p->own_s1, &p->own_put, &p->own_rows})
      HIP_TRY(hipStreamCreateWithFlags(st, hipStreamNonBlocking), "ocean_peers: streams");
    p->row_cus = 0;
  }
  p->s1_stream = p->own_s1;
  p->put_stream = p->own_put;
  p->row_stream = p->own_rows;
  p->put_done_valid[0] = p->put_done_valid[1] = false;
  return OCEAN_OK;
}

void peers_release(ocean_peers* p)
{
  for (hipStream_t st : {p->s1_stream, p->put_stream, p->row_stream})
    if (st)
      (void)hipStreamSynchronize(st);
  if (p->g && p->g->fft)
    (void)hipStreamSynchronize(p->g->fft->stream);
  for (int q = 0; q < kMaxRanks; q++)
  {
    if (p->mapped[q] && p->peer_data[q])
      (void)hipIpcCloseMemHandle(p->peer_data[q]);
    if (p->mapped[kMaxRanks + q] && p->peer_flags[q])
      (void)hipIpcCloseMemHandle(p->peer_flags[q]);
    p->mapped[q] = p->mapped[kMaxRanks + q] = false;
  }
}

// an RCCL pipelined frame in flight lands before a one-sided frame's column pass
int put_frame_start(ocean_generator* g, ocean_peers* p, const char* who)
{
  TRY(check_peers(g, p, who));
  return ocean_generator_slab_flush(g);
}
}  // namespace

extern "C" {

int ocean_peers_create(ocean_peers** out, ocean_generator* g)
{
  if (!out || !g)
    return fail(OCEAN_ERR_INVALID, "ocean_peers_create: null argument");
  *out = nullptr;
  if (!g->slab || !half_slab_path(g))
    return fail(OCEAN_ERR_INVALID, "ocean_peers_create: a slab generator on a half-spectrum path (N >= 1024)");
  if (g->peers)
    return fail(OCEAN_ERR_INVALID, "ocean_peers_create: the generator already has peers");
  HIP_TRY(hslab_buffers(g), "ocean_peers_create: generator buffers");
  auto* p = new ocean_peers();
  p->g = g;
  p->rank = g->rank;
  p->ranks = g->ranks;
  p->slot = hslab_xbuf_bytes(g);
  p->blk = p->slot / g->ranks;
  hipError_t e = hipMalloc(&p->data, 2 * p->slot);
  // the flag words in uncached memory: polled by one wave, written by the peers over xGMI
  if (e == hipSuccess)
  {
    if (hipExtMallocWithFlags((void**)&p->flags, kFlagWords * sizeof(uint32_t), hipDeviceMallocUncached) == hipSuccess)
      p->flags_uncached = true;
    else
    {
      (void)hipGetLastError();
      e = hipMalloc(&p->flags, kFlagWords * sizeof(uint32_t));
    }
  }
  e = alloc_if_null(p->table, 3 * kMaxRanks * sizeof(uint64_t), e);
  if (e == hipSuccess)
    e = hipMemset(p->flags, 0, kFlagWords * sizeof(uint32_t));
  for (hipEvent_t* ev : {&p->s1_done[0], &p->put_done[0], &p->s1_done[1], &p->put_done[1], &p->rows_done, &p->gen_ready})
    if (e == hipSuccess)
      e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
  if (e == hipSuccess)
    e = hipDeviceSynchronize();
  int rc = e == hipSuccess ? peers_deadline(p) : OCEAN_OK;
  if (rc == OCEAN_OK && e == hipSuccess)
    rc = peers_streams(p);
  if (e != hipSuccess || rc != OCEAN_OK)
  {
    p->g = nullptr;
    ocean_peers_destroy(p);
    return rc != OCEAN_OK ? rc : alloc_fail(e, "ocean_peers_create");
  }
  p->peer_data[p->rank] = p->data;
  p->peer_flags[p->rank] = p->flags;
  g->peers = p;
  *out = p;
  return OCEAN_OK;
}

int ocean_peers_destroy(ocean_peers* p)
{
  if (!p)
    return OCEAN_OK;
  peers_release(p);
  if (p->g)
    p->g->peers = nullptr;
  for (hipStream_t st : {p->own_s1, p->own_put, p->own_rows})
    if (st)
      (void)hipStreamDestroy(st);
  for (hipEvent_t ev : {p->s1_done[0], p->put_done[0], p->s1_done[1], p->put_done[1], p->rows_done, p->gen_ready})
    if (ev)
      (void)hipEventDestroy(ev);
  for (void* q : {(void*)p->data, (void*)p->flags, (void*)p->table, (void*)p->parts2})
    if (q)
      (void)hipFree(q);
  delete p;
  return OCEAN_OK;
}

int ocean_peers_handle(const ocean_peers* p, unsigned char handle[OCEAN_PEER_HANDLE_BYTES])
{
  if (!p || !handle)
    return fail(OCEAN_ERR_INVALID, "ocean_peers_handle: null argument");
  PeerHandle h{};
  h.magic = kPeerMagic;
  h.rank = p->rank;
  h.ranks = p->ranks;
  h.flags_uncached = p->flags_uncached ? 1 : 0;
  h.slot_bytes = p->slot;
  HIP_TRY(hipIpcGetMemHandle(&h.data, p->data), "ocean_peers_handle: hipIpcGetMemHandle (slots)");
  HIP_TRY(hipIpcGetMemHandle(&h.flags, p->flags), "ocean_peers_handle: hipIpcGetMemHandle (flags)");
  std::memset(handle, 0, OCEAN_PEER_HANDLE_BYTES);
  std::memcpy(handle, &h, sizeof(h));
  return OCEAN_OK;
}

int ocean_peers_connect(ocean_peers* p, const unsigned char* handles)
{
  if (!p || !handles || !p->g)
    return fail(OCEAN_ERR_INVALID, "ocean_peers_connect: null argument or detached peers");
  if (p->connected)
    return fail(OCEAN_ERR_INVALID, "ocean_peers_connect: already connected");
  for (int q = 0; q < p->ranks; q++)
  {
    PeerHandle h;
    std::memcpy(&h, handles + (size_t)q * OCEAN_PEER_HANDLE_BYTES, sizeof(h));
    if (h.magic != kPeerMagic || h.rank != q || h.ranks != p->ranks || h.slot_bytes != p->slot)
      return fail(OCEAN_ERR_INVALID, "ocean_peers_connect: handle " + std::to_string(q) + " is not rank " +
                                         std::to_string(q) + " of " + std::to_string(p->ranks) +
                                         " with this grid's slot size");
    if (q == p->rank)
      continue;
    void* d = nullptr;
    void* fl = nullptr;
    hipError_t e = hipIpcOpenMemHandle(&d, h.data, hipIpcMemLazyEnablePeerAccess);
    if (e == hipSuccess)
    {
      p->peer_data[q] = static_cast<unsigned char*>(d);
      p->mapped[q] = true;
      e = hipIpcOpenMemHandle(&fl, h.flags, hipIpcMemLazyEnablePeerAccess);
    }
    if (e == hipSuccess)
    {
      p->peer_flags[q] = static_cast<uint32_t*>(fl);
      p->mapped[kMaxRanks + q] = true;
    }
    if (e != hipSuccess)
    {
      peers_release(p);
      return hip_fail(e, ("ocean_peers_connect: hipIpcOpenMemHandle of rank " + std::to_string(q)).c_str());
    }
  }
  return peers_table(p);
}

int ocean_peers_connect_local(ocean_peers* const* all, int ranks)
{
  if (!all || ranks < 1 || ranks > kMaxRanks)
    return fail(OCEAN_ERR_INVALID, "ocean_peers_connect_local: null array or ranks outside [1, 16]");
  for (int q = 0; q < ranks; q++)
    if (!all[q] || !all[q]->g || all[q]->rank != q || all[q]->ranks != ranks || all[q]->slot != all[0]->slot ||
        all[q]->connected)
      return fail(OCEAN_ERR_INVALID, "ocean_peers_connect_local: entry " + std::to_string(q) +
                                         " is not an unconnected rank " + std::to_string(q) + " of " +
                                         std::to_string(ranks) + " of one grid");
  for (int r = 0; r < ranks; r++)
  {
    for (int q = 0; q < ranks; q++)
    {
      all[r]->peer_data[q] = all[q]->data;
      all[r]->peer_flags[q] = all[q]->flags;
    }
    TRY(peers_table(all[r]));
  }
  return OCEAN_OK;
}

int ocean_peers_set_timeout(ocean_peers* p, int ms)
{
  if (!p || ms < 1)
    return fail(OCEAN_ERR_INVALID, "ocean_peers_set_timeout: null peers or ms < 1");
  p->timeout_ms = ms;
  return peers_deadline(p);
}

int ocean_peers_set_put_cus(ocean_peers* p, int cus)
{
  if (!p || !p->g || cus < 0 || cus > p->g->fft->device_cus)
    return fail(OCEAN_ERR_INVALID, "ocean_peers_set_put_cus: null peers or CUs outside [0, device CUs]");
  p->put_cus = cus;
  return OCEAN_OK;
}

int ocean_peers_set_streams(ocean_peers* p, void* column_stream, void* put_stream, void* row_stream)
{
  if (!p || !p->g)
    return fail(OCEAN_ERR_INVALID, "ocean_peers_set_streams: null or detached peers");
  if (p->rows < p->frames)
    return fail(OCEAN_ERR_INVALID, "ocean_peers_set_streams: a pipelined frame is in flight (flush first)");
  for (hipStream_t st : {p->s1_stream, p->put_stream, p->row_stream})
    HIP_TRY(hipStreamSynchronize(st), "ocean_peers_set_streams");
  p->s1_stream = column_stream ? (hipStream_t)column_stream : p->own_s1;
  p->put_stream = put_stream ? (hipStream_t)put_stream : p->own_put;
  p->row_stream = row_stream ? (hipStream_t)row_stream : p->own_rows;
  p->put_done_valid[0] = p->put_done_valid[1] = false;  // the old streams are drained
  return OCEAN_OK;
}

int ocean_peers_set_row_cus(ocean_peers* p, int cus)
{
  if (!p || !p->g || cus < 0)
    return fail(OCEAN_ERR_INVALID, "ocean_peers_set_row_cus: null peers or negative CUs");
  p->caller_row_cus = cus;
  return OCEAN_OK;
}

int ocean_peers_set_put_cu_mask(ocean_peers* p, int cus_per_xcd)
{
  if (!p || !p->g || cus_per_xcd < 0 || cus_per_xcd >= p->g->fft->device_cus / 8)
    return fail(OCEAN_ERR_INVALID, "ocean_peers_set_put_cu_mask: null peers or CUs per XCD outside [0, CUs / 8)");
  if (p->rows < p->frames)
    return fail(OCEAN_ERR_INVALID, "ocean_peers_set_put_cu_mask: a pipelined frame is in flight (flush first)");
  const bool own = p->s1_stream == p->own_s1 && p->put_stream == p->own_put && p->row_stream == p->own_rows;
  if (!own)
    return fail(OCEAN_ERR_INVALID, "ocean_peers_set_put_cu_mask: the caller's streams are in use (ocean_peers_set_streams)");
  p->put_cus_per_xcd = cus_per_xcd;
  return peers_streams(p);
}

int ocean_generator_slab_put_columns(ocean_generator* g, ocean_peers* p, float timestep, int update_spectrum)
{
  TRY(put_frame_start(g, p, "ocean_generator_slab_put_columns"));
  return put_columns(g, p, timestep, update_spectrum, false);
}

int ocean_generator_slab_put_rows(ocean_generator* g, ocean_peers* p)
{
  TRY(check_peers(g, p, "ocean_generator_slab_put_rows"));
  return put_rows(g, p);
}

int ocean_generator_slab_frame_put(ocean_generator* g, ocean_peers* p, float timestep, int update_spectrum)
{
  TRY(put_frame_start(g, p, "ocean_generator_slab_frame_put"));
  while (p->rows < p->frames)  // a pipelined frame in flight lands first
    TRY(put_rows(g, p));
  TRY(put_columns(g, p, timestep, update_spectrum, false));
  return put_rows(g, p);
}

int ocean_generator_slab_frame_put_pipelined(ocean_generator* g, ocean_peers* p, float timestep, int update_spectrum)
{
  TRY(put_frame_start(g, p, "ocean_generator_slab_frame_put_pipelined"));
  TRY(put_columns(g, p, timestep, update_spectrum, true));
  while (p->rows < p->frames - 1)  // frame f - 1's row pass beside frame f's columns
    TRY(put_rows(g, p, true));
  return OCEAN_OK;
}

int ocean_peers_flush(ocean_peers* p)
{
  if (!p || !p->g)
    return fail(OCEAN_ERR_INVALID, "ocean_peers_flush: null or detached peers");
  while (p->rows < p->frames)
    TRY(put_rows(p->g, p, true));
  return OCEAN_OK;
}

int ocean_peers_synchronize(ocean_peers* p)
{
  if (!p)
    return fail(OCEAN_ERR_INVALID, "ocean_peers_synchronize: null peers");
  HIP_TRY(hipStreamSynchronize(p->s1_stream), "ocean_peers_synchronize: column stream");
  HIP_TRY(hipStreamSynchronize(p->put_stream), "ocean_peers_synchronize: put stream");
  HIP_TRY(hipStreamSynchronize(p->row_stream), "ocean_peers_synchronize: row stream");
  if (p->g)
    HIP_TRY(hipStreamSynchronize(p->g->fft->stream), "ocean_peers_synchronize: generator stream");
  uint32_t err = 0;
  HIP_TRY(hipMemcpy(&err, p->flags + kErrWord, sizeof(err), hipMemcpyDeviceToHost), "ocean_peers_synchronize: status");
  if (err != 0)
  {
    // The word is sticky on the device (every later wait returns at once). Now that the streams are
    // drained it is cleared, and the peers refuse further frames (check_peers): after a timeout the
    // ranks' ready / freed counts no longer agree, so the only way on is a new peers object.
    p->failed = true;
    HIP_TRY(hipMemset(p->flags + kErrWord, 0, sizeof(uint32_t)), "ocean_peers_synchronize: clear status");
    HIP_TRY(hipDeviceSynchronize(), "ocean_peers_synchronize: clear status");
    return fail(OCEAN_ERR_TIMEOUT, std::string("one-sided exchange: a wait for the peers' ") +
                                       (err - 1 == kReadyWord ? "blocks (ready)" : "slot release (freed)") +
                                       " timed out after " + std::to_string(p->timeout_ms) +
                                       " ms; the frames since then are invalid, and this peers object refuses new "
                                       "frames");
  }
  return p->failed ? fail(OCEAN_ERR_TIMEOUT, "one-sided exchange: an earlier wait timed out; recreate the peers")
                   : OCEAN_OK;
}

int ocean_peers_debug_slot(const ocean_peers* p, int slot, void** ptr, size_t* bytes)
{
  if (!p || !ptr || !bytes || slot < 0 || slot > 1)
    return fail(OCEAN_ERR_INVALID, "ocean_peers_debug_slot: null argument or slot outside {0, 1}");
  *ptr = p->data + (size_t)slot * p->slot;
  *bytes = p->slot;
  return OCEAN_OK;
}

}  // extern "C"
