/*
 * oceanfft.h — C ABI of the MI355X ocean height-field library (liboceanfft.so).
 *
 * Drop-in boundary for the hot path of James51332/OceanSimulation:
 *   Waves::FFTCalculator  (src/FFTCalculator.h:11-59, src/FFTCalculator.cpp:10-114)
 *   Waves::Generator      (src/Generator.h:33-93,     src/Generator.cpp:14-154)
 *   Waves::GeneratorSettings (src/Generator.h:12-30)
 * Every entry point below cites the reference member it replaces. The C++ classes with the
 * reference's exact signatures (include/waves/Generator.h, FFTCalculator.h) are thin wrappers over this ABI; INTEGRATION.md
 * shows the ctypes/C++ bindings.
 *
 * Conventions
 *   - Plain C types only. Device buffers are `float*` into HBM: RGBA32F images are N*N float4,
 *     row-major, x fastest (image x = column, resources/fft.compute:72-73); R32F maps are N*N float.
 *   - Every function returns an int status (OCEAN_OK == 0) unless it is a getter; on failure
 *     ocean_last_error() gives a thread-local message. (The reference has no error path at all —
 *     its calls are void and misuse such as N != SIZE silently corrupts results; here misuse fails.)
 *   - One context per HIP stream: all work of an ocean_fft and of the generators bound to it is
 *     issued on the stream given at ocean_fft_create (nullptr = the default stream). Calls only
 *     enqueue work (the reference's "encode into a command buffer"); ocean_fft_synchronize waits.
 *   - Library-owned outputs are borrowed by the caller and valid until the owner is destroyed
 *     (the reference's Vision::ID handles, src/Generator.h:48-50).
 */
#ifndef OCEANFFT_H
#define OCEANFFT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OCEAN_OK 0
#define OCEAN_ERR_INVALID 1   /* bad argument (size not a power of two in [16, 16384], null, range) */
#define OCEAN_ERR_HIP 2       /* HIP runtime error (message in ocean_last_error) */
#define OCEAN_ERR_NO_DEVICE 3 /* no GPU visible */
#define OCEAN_ERR_OOM 4       /* device allocation failed */
/* OCEAN_ERR_TIMEOUT 5: see the one-sided slab exchange below */

#define OCEAN_MAX_CASCADES 64

/* Waves::GeneratorSettings (src/Generator.h:12-30); same 64-byte layout as the std140 UBO
 * spectrumSettings (resources/spectrum.compute:10-27). */
typedef struct ocean_settings
{
  int32_t seed[2];         /* seed for the hash noise */
  float U_10;              /* wind speed */
  float theta_0;           /* wind direction (the reference subtracts it from radians as-is) */
  float F;                 /* fetch */
  float g;                 /* gravity */
  float swell;             /* swell factor */
  float h;                 /* depth */
  float displacement;      /* choppiness lambda used by the Jacobian */
  float time;              /* seconds, accumulated in fp32 by calculate() */
  float planeSize;         /* metres covered by the tile */
  float scale;             /* global amplitude scale */
  float spread;            /* directional spread blend */
  int32_t boundWavelength; /* uploaded but unused by the reference (spectrum.compute:24) */
  float wavelengthMin;     /* idem */
  float wavelengthMax;     /* idem */
} ocean_settings;

typedef struct ocean_fft ocean_fft;             /* Waves::FFTCalculator */
typedef struct ocean_generator ocean_generator; /* one or more Waves::Generator cascades */

/* ---- library ---------------------------------------------------------------------------- */
const char* ocean_last_error(void);
const char* ocean_version(void);
/* GeneratorSettings default member initialisers, src/Generator.h:14-29. */
void ocean_default_settings(ocean_settings* s);
/* Number of visible GPUs (0 when none); does not create a context. */
int ocean_device_count(void);

/* ---- FFTCalculator ------------------------------------------------------------------------ */
/* FFTCalculator::FFTCalculator(RenderDevice*, size_t textureSize) — src/FFTCalculator.cpp:10-58.
 * Builds the twiddle table on the device; texture_size must be a power of two in [16, 16384]. */
int ocean_fft_create(ocean_fft** out, size_t texture_size, void* hip_stream);
/* FFTCalculator::~FFTCalculator — src/FFTCalculator.cpp:61-71. */
int ocean_fft_destroy(ocean_fft* fft);
/* FFTCalculator::GetTextureResolution — src/FFTCalculator.h:24. */
size_t ocean_fft_texture_resolution(const ocean_fft* fft);
/* FFTCalculator::EncodeIFFT(Vision::ID image) — src/FFTCalculator.cpp:73-114. In place on a
 * device RGBA32F N*N image: out = N^2 * ifft2(ifftshift(in)) on lanes xy and zw independently
 * (no normalisation, like the reference). The caller needs no work image; the plan allocates its
 * own on first use where a faster order needs one (N = 4096: column-first through up to 8 images;
 * N = 16384: rows, then a four-step column transform through an N x 2048 slab), and falls back to
 * the in-place passes when that allocation fails. */
int ocean_fft_encode_ifft(ocean_fft* fft, float* image);
/* Batched EncodeIFFT over n_images contiguous images (image i at image + i*N*N*4 floats). */
int ocean_fft_encode_ifft_batch(ocean_fft* fft, float* images, int n_images);
/* Wait for all work enqueued on the plan's stream (the reference's SubmitCommandBuffer + fence,
 * src/Waves.cpp:106). */
int ocean_fft_synchronize(ocean_fft* fft);
/* Multiprocessor (CU) count of the plan's device. */
int ocean_fft_device_cus(const ocean_fft* fft);
/* Size the plan's persistent grids (every kernel of this plan and its generators) for `cus` CUs
 * instead of all of them (0 restores all). The frame kernels take a whole CU per workgroup, so a
 * budget below the device count leaves CUs free for work on other streams, e.g. the copy kernels
 * of an RCCL all-to-all overlapped with the slab passes. No reference counterpart. */
int ocean_fft_set_cu_budget(ocean_fft* fft, int cus);

/* ---- Generator ---------------------------------------------------------------------------- */
/* Generator::Generator(RenderDevice*, FFTCalculator*) — src/Generator.cpp:14-27, batched over
 * `cascades` independent cascades (1..OCEAN_MAX_CASCADES) that share the plan's size N. Allocates
 * per cascade: initialSpectrum, heightMap, displacementMap (RGBA32F N*N) and jacobian (R32F N*N)
 * (src/Generator.cpp:99-133). Settings start at the defaults; the first calculate() seeds h0. */
int ocean_generator_create(ocean_generator** out, ocean_fft* fft, int cascades);
/* Generator::~Generator — src/Generator.cpp:29-43 (also frees the jacobian the reference leaks). */
int ocean_generator_destroy(ocean_generator* gen);
int ocean_generator_cascades(const ocean_generator* gen);
/* Generator::GetOceanSettings — src/Generator.h:41. Host-side, mutable; read at calculate(). */
ocean_settings* ocean_generator_settings(ocean_generator* gen, int cascade);
/* Generator::CalculateOcean(float timestep, bool updateOcean) — src/Generator.cpp:45-83, for all
 * cascades: time += timestep (fp32); regenerate h0 when update_spectrum != 0 or on first use;
 * evolve + pack + two EncodeIFFTs + foam. Two fused launches: column pass (evolve + y iFFT of
 * both packed maps) and row pass (x iFFT + row-major maps + Jacobian). */
int ocean_generator_calculate(ocean_generator* gen, float timestep, int update_spectrum);
/* Generator::GenerateSpectrum — src/Generator.cpp:148-154 (the generateSpectrum dispatch). */
int ocean_generator_generate_spectrum(ocean_generator* gen);
/* Getters — src/Generator.h:48-50. Device pointers; heightMap = (h, dh/dx, dh/dz, Dx),
 * displacementMap = (Dz, dDx/dx, dDz/dz, dDx/dz) (src/Generator.h:76-80), jacobian = R32F. */
float* ocean_generator_height_map(ocean_generator* gen, int cascade);
float* ocean_generator_displacement_map(ocean_generator* gen, int cascade);
float* ocean_generator_jacobian_map(ocean_generator* gen, int cascade);
/* The initialSpectrum image (private in the reference, src/Generator.h:86): (h0(k), conj(h0(-k)))
 * per texel, stored strip-blocked: texel (x, y) at index ((x / B) * N + y) * B + (x % B) with
 * B = ocean_generator_spectrum_block(gen), so the column pass streams it contiguously. Slab
 * generators hold only their own columns: the column slab (full spectrum), their kept strips in
 * order, each N * B texels (strip-dealt half spectrum; the Nyquist strip x = 0 .. B-1 last), or their
 * kept columns x = N/2 + u0 .. blocked 64 wide from u0, the last rank then the block of x = 0 .. 63
 * (four-step, ocean_slab_layout half == 2). The pointer is writable: see ocean_generator_set_h0_memo. */
float* ocean_generator_initial_spectrum(ocean_generator* gen, int cascade);
int ocean_generator_spectrum_block(const ocean_generator* gen);

/* Frame path. Half spectrum (default for N = 1024 .. 16384): the column pass transforms only the
 * u >= 0 half of the columns, as 5 complex fields (H, kz H, H/|k|, kz H/|k|, kz^2 H/|k|), and the
 * row pass rebuilds the reference's 4 packed lanes from Hermitian symmetry plus the reference's
 * Nyquist-row term. Whole grids of 1024 .. 4096 use the blocked layout (84 HBM bytes
 * per point instead of 116). N = 8192 / 16384 (whole grids and slabs) run the four-step column pass,
 * whose second step writes destination-block order, so the row pass reads the exchanged blocks
 * directly (124 bytes per point; exchange 20 bytes per point instead of 32); slabs of 1024 .. 4096
 * deal the kept strips over the ranks and move the received fields to row-major before the row pass.
 * enable = 0 selects the full-spectrum path (both give the reference's results within rounding). On a
 * slab generator the switch changes ocean_generator_exchange_bytes and re-seeds h0 at the next frame. */
int ocean_generator_set_half_spectrum(ocean_generator* gen, int enable);
/* N = 8192 / 16384, half spectrum (whole grids and slabs): enable (default) = the column pass in four
 * steps (N = 16 * N2: a 16-point step in registers, then N2-point transforms on 8-column strips
 * written straight into destination-block order; no one-column work items and no transposes; h0 is
 * then blocked ocean_generator_spectrum_block = 64 columns wide, a slab holding only its own kept
 * columns); 0 = the strip-dealt column pass + transposes into row-major fields. Both give the
 * reference's results within rounding. Switching changes ocean_generator_exchange_bytes and re-lays h0
 * out at the next frame from the settings it was seeded with. No reference counterpart. */
int ocean_generator_set_four_step(ocean_generator* gen, int enable);
/* A re-seed requested by ocean_generator_calculate(.., update_spectrum = 1) — the reference app
 * requests one on every frame (src/Waves.cpp:91-94) — is skipped when no h0 input (every settings
 * field but `time`) changed since h0 was last seeded: it would reproduce the same image bit for bit.
 * Handing out the h0 pointer (ocean_generator_initial_spectrum) makes the next requested re-seed run,
 * since the caller may have written h0 through it. enable = 0 re-seeds on every request, as the
 * reference does. Default 1. No reference counterpart. */
int ocean_generator_set_h0_memo(ocean_generator* gen, int enable);
/* Frame overlap (whole grids of N = 1024 .. 4096 on the half-spectrum path): frame f + 1's column
 * pass, which depends only on h0 and the time, runs on an internal stream into a second set of field
 * buffers while frame f's row pass still runs on the generator's stream, so the two passes' launch
 * tails overlap when the caller issues frames back to back. Row passes, maps and Jacobian stay in
 * order on the generator's stream, and the results are bit-identical. The internal stream waits for
 * the generator's stream whenever the library writes h0 (seeding, re-seeds) and after the h0 pointer
 * is handed out (ocean_generator_initial_spectrum); other work the caller enqueues on that stream
 * between frames is not waited for, so it must not write the generator's buffers. Costs 20 B of
 * device memory per point. Pays at 1-2 cascades per generator of 1024^2 (8 x 4096^2: slower, leave it
 * off). At 2048 and 4096 with 1-2 cascades the column pass runs on half strips, which share CUs with
 * the overlapped row pass: there the serial frame is faster (0.318 against 0.346 ms at one cascade of
 * 4096, profiles/r04_halfbench_xgrid_fb2_1.log; 0.087 against 0.091 ms at one of 2048,
 * profiles/r06g_configs.md), so leave it off as well.
 * Default 0. No reference counterpart (the reference barriers after every dispatch). */
int ocean_generator_set_frame_overlap(ocean_generator* gen, int enable);
/* Algorithmic HBM bytes per height-field point of the column pass [0] and the row pass [1] of the
 * generator's current path (what bench.py prices the roofline with). */
int ocean_generator_frame_bytes(const ocean_generator* gen, double per_point[2]);

/* ---- slab decomposition of one grid over several GPUs ------------------------------------- */
/* One N x N cascade split over `ranks` GPUs (power of two <= 16), this process being `rank`: the
 * column pass works on columns [rank*w, rank*w + w), the row pass on rows [rank*w, rank*w + w),
 * w = N / ranks (the reference runs everything on one device). With the half spectrum
 * (default for N >= 1024) the column pass works on the rank's share of the kept strips instead of
 * the column slab. A frame is:
 *   ocean_generator_slab_columns(gen, dt, update, send)  time += dt, h0 if needed, evolve + y iFFT
 *   all-to-all with equal splits of ocean_generator_exchange_bytes(gen) / ranks bytes: the block at
 *     send + q * bytes/ranks goes to rank q and arrives at recv + rank_src * bytes/ranks (RCCL)
 *   ocean_generator_slab_rows(gen, recv)                 x iFFT + maps + Jacobian of the row slab
 * send/recv are caller-owned device buffers (null = the generator's internal buffer, which is what
 * ranks == 1 uses). The map getters then address the row slab: w rows x N texels, row-major. */
int ocean_generator_create_slab(ocean_generator** out, ocean_fft* fft, int rank, int ranks);
size_t ocean_generator_exchange_bytes(const ocean_generator* gen);
int ocean_generator_slab_columns(ocean_generator* gen, float timestep, int update_spectrum, float* send);
int ocean_generator_slab_rows(ocean_generator* gen, const float* recv);
int ocean_generator_slab_info(const ocean_generator* gen, int* rank, int* ranks, int* row0, int* rows);
/* Host-only geometry of a one-cascade slab generator (no device needed): out = {first kept strip,
 * strips this rank transforms, strip slots per block, rows per block (N / ranks), exchange block
 * bytes, exchange bytes} for the strip-dealt half-spectrum path (half == 1: the STRIPS = N / (2B) + 1
 * kept strips dealt ceil(STRIPS / ranks) per rank); {first kept column u0, kept columns N / (2 ranks),
 * 1 if the rank also holds the Nyquist column, rows, block bytes, exchange bytes} for the four-step
 * path (half == 2, N = 8192 / 16384: the default there); or {first column, columns, 0, rows, block
 * bytes, exchange bytes} for the full-spectrum path (half == 0). */
int ocean_slab_layout(size_t texture_size, int rank, int ranks, int half, int64_t out[6]);

/* ---- the slab exchange over RCCL (xGMI) ---------------------------------------------------
 * The frame of a slab generator with the all-to-all inside the library: P grouped ncclSend /
 * ncclRecv pairs of exchange_bytes / P between the column and the row pass, on the
 * generator's stream (serial) or on a second stream (pipelined). The communicator spans the P ranks
 * of the grid, rank r = the slab rank (one process per GPU, the current HIP device). */
#define OCEAN_COMM_ID_BYTES 128
typedef struct ocean_comm ocean_comm;
/* ncclGetUniqueId: created by one rank and handed to every rank's ocean_comm_create by the caller
 * (MPI, a file, torch.distributed ...). */
int ocean_comm_unique_id(unsigned char id[OCEAN_COMM_ID_BYTES]);
/* ncclCommInitRank(nranks, id, rank) on the current device; collective over the nranks processes. */
int ocean_comm_create(ocean_comm** out, const unsigned char id[OCEAN_COMM_ID_BYTES], int nranks, int rank);
/* Use a communicator the caller already has (an ncclComm_t; not destroyed by ocean_comm_destroy).
 * nranks / rank must be the communicator's own (ncclCommCount / ncclCommUserRank), else
 * OCEAN_ERR_INVALID. A communicator must outlive every generator whose frames used it: destroying
 * a generator drains its exchange stream but does not issue a pending pipelined frame's row pass. */
int ocean_comm_wrap(ocean_comm** out, void* nccl_comm, int nranks, int rank);
int ocean_comm_destroy(ocean_comm* comm);
/* The equal-split all-to-all of caller device buffers over the communicator (bytes / nranks to each
 * rank), enqueued on hip_stream: for callers that run ocean_generator_slab_columns / _rows themselves. */
int ocean_comm_all_to_all(ocean_comm* comm, const void* send, void* recv, size_t bytes, void* hip_stream);
/* One frame: time += dt, h0 if needed, column pass into the library's send buffer, the all-to-all,
 * row pass — all enqueued on the generator's stream (src/Generator.cpp:45-83 over P ranks). */
int ocean_generator_slab_frame(ocean_generator* gen, ocean_comm* comm, float timestep, int update_spectrum);
/* Pipelined frames over two buffer slots: frame f's all-to-all runs on a second stream beside frame
 * f + 1's column pass and frame f - 1's row pass, so the steady state is max(exchange, passes); the
 * maps lag the last issued frame by one until ocean_generator_slab_flush. Size the passes with
 * ocean_fft_set_cu_budget to leave CUs to RCCL's kernels. */
int ocean_generator_slab_frame_pipelined(ocean_generator* gen, ocean_comm* comm, float timestep, int update_spectrum);
int ocean_generator_slab_flush(ocean_generator* gen);

/* ---- the one-sided slab exchange over peer-mapped memory (IPC, xGMI) -----------------------
 * No send buffer and no copy kernel: the column pass's second step stores block q of its output
 * straight into rank q's receive slot, through a mapping of rank q's device memory (hipIpc handles
 * exchanged by the caller), and the row pass reads its own slot. Per frame each rank raises one
 * flag word in every rank's flag array after its stores ("ready") and one after its row pass has
 * read its slot ("freed"); the waits for them are small kernels on the streams (one wave per workgroup,
 * dealt over every XCD, each ending in a system-scope acquire), bounded by a
 * timeout (ocean_peers_set_timeout), so a missing peer never holds the GPU: the frame goes on, and
 * ocean_peers_synchronize reports OCEAN_ERR_TIMEOUT. Every half-spectrum slab path (N >= 1024): on the
 * four-step slabs (N = 8192 / 16384) step 2 puts, on the strip-dealt ones the column pass itself; the
 * RCCL exchange above also serves the full-spectrum slabs below 1024. SURVEY §8e, the reference's
 * CalculateOcean (src/Generator.cpp:45-83) split over P ranks.
 * Use: ocean_peers_create on every rank, ocean_peers_handle -> the caller gathers the P handles (in
 * rank order, e.g. an all-gather) -> ocean_peers_connect; frames; ocean_peers_synchronize on every
 * rank and a host barrier across ranks before ocean_peers_destroy (a peer may still signal). */
#define OCEAN_ERR_TIMEOUT 5   /* a peer's frame signal did not arrive within the timeout */
#define OCEAN_PEER_HANDLE_BYTES 256
typedef struct ocean_peers ocean_peers;
/* Two receive slots of ocean_generator_exchange_bytes(gen) and the flag words, in this process's
 * device memory; gen must be a slab generator on a half-spectrum path (N >= 1024). A later path switch
 * that changes the exchange size makes the peers refuse frames. */
int ocean_peers_create(ocean_peers** out, ocean_generator* gen);
int ocean_peers_destroy(ocean_peers* peers);
/* This rank's handle (rank, ranks, slot size, the IPC handles of its slots and flags). */
int ocean_peers_handle(const ocean_peers* peers, unsigned char handle[OCEAN_PEER_HANDLE_BYTES]);
/* Map every other rank's slots and flags: handles = ranks * OCEAN_PEER_HANDLE_BYTES, in rank order
 * (this rank's own entry is checked and used locally). */
int ocean_peers_connect(ocean_peers* peers, const unsigned char* handles);
/* The same for `ranks` ocean_peers of one process on one device (the single-GPU emulation of a P-rank
 * grid, tests): each rank's peers are the others' buffers directly, no IPC. */
int ocean_peers_connect_local(ocean_peers* const* all, int ranks);
/* Wait timeout in milliseconds (default 20000). */
int ocean_peers_set_timeout(ocean_peers* peers, int ms);
/* CUs the put kernels (the Nyquist-row term and step 2) are sized for (0 = the plan's budget): with
 * the stores bound by xGMI, fewer workgroups leave the other CUs to the row pass of the previous
 * frame in the pipelined frame. */
int ocean_peers_set_put_cus(ocean_peers* peers, int cus);
/* The streams pipelined frames run step 1 of the column pass, the put and the row pass on (null: the
 * peers' own; the generator's stream waits for each row pass, so the maps stay ordered on it). The
 * one-GPU emulation gives all P ranks one set, as one GPU has one path out over xGMI. */
int ocean_peers_set_streams(ocean_peers* peers, void* column_stream, void* put_stream, void* row_stream);
/* The CUs the caller's row stream may use when it is CU-masked (0 = all, the default; the peers' own
 * masked streams know theirs): the 16384 row pass loops over rows on a resident grid, one workgroup per
 * CU, so a grid sized for CUs the stream cannot use leaves whole workgroups waiting for a second turn. */
int ocean_peers_set_row_cus(ocean_peers* peers, int cus);
/* Recreate the peers' own streams CU-masked: the put on `cus_per_xcd` CUs of every XCD, step 1 and the
 * row pass on the others (0: unmasked, the default). An xGMI-bound put then holds only its own CUs
 * while it waits on the links. (A CU mask splits every XCD alike: workgroups are dealt to all 8 XCDs
 * whatever the mask, and an XCD left without mask bits runs on all its CUs.) */
int ocean_peers_set_put_cu_mask(ocean_peers* peers, int cus_per_xcd);
/* Serial frame on the generator's stream: time += dt, h0 if needed, step 1, wait for the slot, put,
 * signal; wait for every rank's blocks, row pass, signal. */
int ocean_generator_slab_frame_put(ocean_generator* gen, ocean_peers* peers, float timestep, int update_spectrum);
/* Pipelined: frame f's step 1 on the peers' column stream (into one of two parts slots), its put on
 * their put stream, beside frame f + 1's step 1 and frame f - 1's row pass on the generator's stream
 * (two receive slots); the maps lag by one frame until ocean_peers_flush. */
int ocean_generator_slab_frame_put_pipelined(ocean_generator* gen, ocean_peers* peers, float timestep,
                                             int update_spectrum);
int ocean_peers_flush(ocean_peers* peers);
/* The two halves of a serial frame, for callers (and the one-GPU emulation) that issue the column
 * passes of all ranks before their row passes: columns + put + signal; wait + rows + signal. */
int ocean_generator_slab_put_columns(ocean_generator* gen, ocean_peers* peers, float timestep, int update_spectrum);
int ocean_generator_slab_put_rows(ocean_generator* gen, ocean_peers* peers);
/* Wait for this rank's streams; OCEAN_ERR_TIMEOUT when any wait gave up (which, and at which frame,
 * in ocean_last_error). After a timeout the device-side error word is cleared and the peers refuse every
 * further frame with OCEAN_ERR_TIMEOUT (the ranks' flag counts no longer agree): destroy and recreate
 * them. Pipelined row passes wait for the caller's work on the generator's stream before they rewrite
 * the maps, and h0 re-seeds wait for the column pass still reading h0 on the peers' streams. */
int ocean_peers_synchronize(ocean_peers* peers);

/* Receive slot `slot` (0 or 1) of this rank: its device pointer and size (frame f's blocks land in
 * slot f % 2). Debug only (tests/test_gpu_peers.py reads a slot into every XCD's L2 just before the
 * peers' put rewrites it, to check that the row pass never reads a stale line). No reference counterpart. */
int ocean_peers_debug_slot(const ocean_peers* peers, int slot, void** ptr, size_t* bytes);

/* The whole-grid half-spectrum frame's layout pairing (N = 1024 .. 4096), host only: out = the field
 * strip width, gab/gde row group, gc row group and h0 strip width the column pass WRITES / reads {0..3},
 * the first three as the row pass READS them {4..6}, and the h0 strip width the seeding writes {7}.
 * Both halves are the members of the shape types the launchers instantiate their kernels from
 * (tests/test_capi_cpu.py checks the pairs over every shape). */
int ocean_frame_plan(size_t texture_size, int cascades, int32_t out[8]);

/* ---- instrumentation (bench) ------------------------------------------------------------- */
/* When enabled, each kernel launch of the generator is bracketed by HIP events on its stream. */
int ocean_generator_set_profiling(ocean_generator* gen, int enable);
/* Synchronises, then returns per-kernel totals since the last call and resets them.
 * Index 0 = spectrum (h0), 1 = column pass (evolve + y iFFT), 2 = row pass (x iFFT + foam). */
int ocean_generator_kernel_times(ocean_generator* gen, double ms_total[3], int64_t launches[3]);
/* The same with index 3 = the put of one-sided frames (the slot wait + the Nyquist-row term + step 2).
 * Index 1 includes it in serial frames; in pipelined ones index 1 is step 1 alone (its own stream). */
int ocean_generator_kernel_times4(ocean_generator* gen, double ms_total[4], int64_t launches[4]);

/* ---- debug -------------------------------------------------------------------------------- */
/* Device Hash (resources/spectrum.compute:109-117) of count (x, y) pairs in device memory:
 * raw[i] = uint32 n, uv[2i..2i+1] = the two uniforms. For bit-exact parity tests. */
int ocean_debug_hash(const uint32_t* xy, int count, uint32_t* raw, float* uv, void* hip_stream);
/* Copy `bytes` (a multiple of 16, 16-B aligned device pointers) with exactly `workgroups` 256-thread
 * workgroups on hip_stream: a rate-limited HBM read + write stream (bench.py prices a slab rank's
 * exchange traffic with it on one GPU). No reference counterpart. */
int ocean_debug_copy(void* dst, const void* src, size_t bytes, int workgroups, void* hip_stream);
/* Cap the EncodeIFFT work image / work slab of this plan at `bytes`: the plan never allocates or keeps
 * one larger than that. An allocation above the cap is not attempted and counts as failed, so the
 * transform takes the documented fallback (with no work image at all: the in-place row and column
 * passes); a work image already held and larger than the cap is freed after the plan's stream drains.
 * Default: (size_t)-1, no cap. For tests of the in-place fallback; no other effect. */
int ocean_debug_fft_work_limit(ocean_fft* fft, size_t bytes);

/* ---- Surface consumer: the renderer's use of the maps -------------------
 * resources/waveShader.glsl evaluated per mesh vertex on the maps of `count` (generator, cascade)
 * pairs (the reference binds 3 generators, src/Renderer.cpp:62-72; here 1..16, one map size,
 * whole-grid generators): the vertex stage's displacement loop (:101-110; cascade i samples at the
 * position cascades < i displaced), then at the displaced position the fragment stage's slope
 * normal and Jacobian average (:127-144). Sampling is GL_LINEAR + GL_REPEAT in fp32
 * (src/Generator.cpp:116-119). Output per vertex: 8 floats (x, y, z, jacobian, nx, ny, nz, 0),
 * device memory, written on the first generator's stream. planeSize / displacement come from each
 * cascade's settings (Renderer.cpp:70-71). A request of at least 65536 vertices and 4 per map
 * texel first repacks the channels each stage reads into an atlas (2 x 16 B per texel and cascade,
 * at most 256 MiB, owned by the first generator's FFT plan and kept for later requests), then samples
 * it: the same bits, fewer load instructions. No reference counterpart as a call: it replaces the
 * vertex + fragment shader sampling. */
int ocean_surface_sample(ocean_generator* const* gens, const int* cascades, int count, const float* xz,
                         int64_t points, float* out);
/* The same on the reference's plane mesh (40 m x 40 m, res x res quads, (res+1)^2 vertices, x
 * fastest; src/Renderer.cpp:18) through the camera-relative warp of waveShader.glsl:77-98:
 * camera = {viewInverse[3].x, .y, .z, forward.x, forward.z} with forward = -viewInverse[0]. */
int ocean_surface_sample_plane(ocean_generator* const* gens, const int* cascades, int count, const float camera[5],
                               int res, float* out);
/* The opposite direction: the water surface above world positions. ocean_surface_sample carries a
 * base point p to V(p) = (p.x + sum scale*Dx, sum h, p.z + sum scale*Dz, ...)
 * (waveShader.glsl:101-110); a floating body asks which p lands on its q = (x, z), i.e. inverts the horizontal displacement.
 * Per point, with V(p) the 8 floats ocean_surface_sample returns for base position p, all in
 * unfused fp32:
 *     p = q
 *     repeat at most `iterations` times:
 *         r = q - (V(p)[0], V(p)[2])
 *         if max(|r.x|, |r.z|) <= tolerance: stop
 *         p = p + r
 *     V = V(p)
 *     out = (p.x, V[1], p.z, V[3],  V[4], V[5], V[6],  max(|q.x - V[0]|, |q.z - V[2]|))
 * Slots 0, 2: the recovered base point; 1: the water height above q; 3 and 4-6: the Jacobian
 * average and the slope normal at the displaced position (the fragment stage, :127-144, unchanged);
 * 7: the residual in metres (ocean_surface_sample leaves this slot 0). iterations == 0 is the
 * forward sample at q with the residual filled in. This is the plain fixed point: it converges
 * where the displacement is a contraction (roughly, where the Jacobian stays well above 0) and does
 * not converge on folded crests, where it oscillates. The call does not fail there: the residual
 * tells the caller, point by point. xz: points x 2 floats, out: points x 8 floats, device memory;
 * (generator, cascade) rules and stream as ocean_surface_sample; the same atlas, which pays
 * sooner here (up to iterations + 1 samplings per point): from 16384 points and one point per 48
 * map texels at 2 or more iterations, from 65536 and one per 24 below. The same bits either way.
 * OCEAN_ERR_INVALID, before any device call: null gens / cascades, iterations outside 0..64, a
 * negative or non-finite tolerance, negative points, null xz / out with points > 0. points == 0
 * launches nothing.
 * No reference counterpart. */
int ocean_surface_query(ocean_generator* const* gens, const int* cascades, int count, const float* xz,
                        int64_t points, int iterations, float tolerance, float* out);

/* ---- Mip pyramids of the maps and footprint-aware sampling ----------------------------------
 * The calls above sample level 0 with GL_LINEAR, like the reference (src/Generator.cpp:116-119 builds
 * no mip chain). That is right while neighbouring samples sit about a texel apart; the reference's own
 * mesh (waveShader.glsl:95 stretches the plane by pow(len, 1.2) * camY * 0.04) puts them tens to
 * thousands of texels apart, where point samples of the maps alias and shimmer from frame to frame.
 * These calls build the box-filter pyramid of glGenerateMipmap and sample it by a per-point footprint.
 *
 * The pyramid, per map of a cascade (heightMap, displacementMap: RGBA32F; jacobian: R32F) and per
 * channel, in fp32: level 0 is the map, level l + 1 has side N >> (l + 1) and
 *     L[l+1](x, y) = 0.25f * ((L[l](2x, 2y) + L[l](2x+1, 2y)) + (L[l](2x, 2y+1) + L[l](2x+1, 2y+1)))
 * from the rounded level below, down to 1 x 1: log2(N) + 1 levels. The sum order is part of the
 * contract (the result is bit for bit this formula however the levels are fused). */
/* log2(N) + 1; 0 for a null generator. */
int ocean_generator_mip_levels(const ocean_generator* gen);
/* Enqueue, on the generator's stream, the rebuild of the levels >= 1 of all three maps of every
 * cascade from the current maps: ceil(log2(N) / 6) kernel launches, 36 B read and 12 B written per
 * point. The storage (a third of the maps', about 12 B per point) is allocated on the first call
 * (OCEAN_ERR_OOM when that fails) and freed by ocean_generator_destroy. Whole-grid generators only:
 * a slab generator gets OCEAN_ERR_INVALID before any device call. The pyramid is fresh until the next
 * call that rewrites the maps (ocean_generator_calculate and the other frame calls); the library
 * tracks that on the host. No reference counterpart. */
int ocean_generator_build_mips(ocean_generator* gen);
/* Level `level` of a cascade's map: level 0 is the map itself (ocean_generator_height_map, ...), a
 * level >= 1 a row-major image of side N >> level in the pyramid's storage, valid until the generator
 * is destroyed and holding what the last ocean_generator_build_mips wrote. Null, with
 * ocean_last_error set, for a null generator, a cascade or level out of range, or a level >= 1 of a
 * pyramid that was never built. */
float* ocean_generator_height_mip(ocean_generator* gen, int cascade, int level);
float* ocean_generator_displacement_mip(ocean_generator* gen, int cascade, int level);
float* ocean_generator_jacobian_mip(ocean_generator* gen, int cascade, int level);
/* ocean_surface_sample with a footprint per point: xzf holds points x 3 floats (x, z, footprint) in
 * device memory, the footprint being the spacing in metres between this sample and its neighbours.
 * Per point and cascade c, in unfused fp32, with top = log2(N):
 *     r = (footprint * (float)N) / planeSize_c
 *     if   !(r >= 1.0f)           : l = 0,   f = 0        (also NaN, negative, 0)
 *     elif r >= (float)(1 << top) : l = top, f = 0        (also +inf)
 *     else l = floor(log2 r) (r's exponent), f = r * 2^-l - 1.0f     (exact, in [0, 1))
 *     value = A when f == 0, else A + f * (B - A)
 * A: the GL_LINEAR + GL_REPEAT sample of level l (side N >> l), B: of level l + 1. The blend is linear
 * in the footprint and continuous across levels. The vertex stage reads h, Dx, Dz with cascade c's
 * (l, f); the fragment stage reads the four slopes and the Jacobian with the same (l, f) at the
 * displaced position; accumulation, normal and Jacobian average are those of ocean_surface_sample, so
 * footprint 0 gives its bits. Output: its 8 floats with slot 7 = the footprint as given.
 * Argument rules, (generator, cascade) rules and stream as ocean_surface_sample; no atlas. Every
 * generator's pyramid must be built and fresh: otherwise OCEAN_ERR_INVALID, naming the index of the
 * generator in `gens`, before any device call. No reference counterpart. */
int ocean_surface_sample_lod(ocean_generator* const* gens, const int* cascades, int count, const float* xzf,
                             int64_t points, float* out);
/* ocean_surface_sample_plane with the footprint the warp gives each vertex: the plane's quad size
 * times the vertex's warp factor, footprint = k * (40.0f / (float)res) with
 * k = powf(max(len, 1), 1.2f) * max(camera.y, 10) * 0.04f as the warp computes it. Slot 7 = that
 * footprint. */
int ocean_surface_sample_plane_lod(ocean_generator* const* gens, const int* cascades, int count,
                                   const float camera[5], int res, float* out);

/* ---- Time derivative of the maps and the velocity of water particles --------------------------
 * The calls above say where the water is; these say how it moves (drag and added mass on a floating
 * body's hull points, motion vectors, spray). Differencing two extra frames at t +- delta costs two
 * frames and fails at large t, where the phase w * t is rounded to fp32 and the maps are not smooth in
 * t. The derivative is analytic where the frame evolves the spectrum: with (a, b) the h0 texel,
 *     H(k, t) = a e^{iwt} + b e^{-iwt},     dH/dt = i w (a e^{iwt} - b e^{-iwt}),
 * and everything after H is linear and independent of t.
 *
 * Contract, per cascade and texel (x, y), in fp32: a = the h0 texel, k = |kvec(x, y)| + 1e-6,
 * w = dispersion(k), (s, c) = sin / cos of w * time, with dk, time, g and h the values the last column
 * pass used (so w and the phase have the frame's bits);
 *     D  = a.xy * (c + i s) - a.zw * (c - i s),     Hd = i w D = (-w D.y, w D.x).
 * The two images are prepareFFT's packing (spectrum.compute:236-237) with H replaced by Hd, each run
 * through EncodeIFFT. Because the packing is the frame's own, Nyquist-row defect included, the result is
 * the exact time derivative of all eight channels of the maps as the library shows them:
 *     height-rate       = d/dt (h, dh/dx, dh/dz, Dx)
 *     displacement-rate = d/dt (Dz, dDx/dx, dDz/dz, dDx/dz)
 * Enqueued on the generator's stream: one packing kernel (16 B read, 32 B written per point) and one
 * batched EncodeIFFT over the 2 * cascades images, about twice a frame's traffic. The storage
 * (32 B per point and cascade) is allocated on the first call (OCEAN_ERR_OOM when that fails) and freed
 * by ocean_generator_destroy. Whole-grid generators only, every N in 16 .. 16384: a slab generator gets
 * OCEAN_ERR_INVALID before any device call, and so does a generator that has calculated no frame yet.
 * The rates are fresh until the next frame call (its column pass moves the time); the library tracks
 * that on the host. No reference counterpart. */
int ocean_generator_calculate_rates(ocean_generator* gen);
/* RGBA32F N*N, row-major, valid until the generator is destroyed and holding what the last
 * ocean_generator_calculate_rates wrote. Null, with ocean_last_error set, for a null generator, a
 * cascade out of range, or rates that were never calculated. */
float* ocean_generator_height_rate_map(ocean_generator* gen, int cascade);
float* ocean_generator_displacement_rate_map(ocean_generator* gen, int cascade);
/* The velocity of the water particle whose rest position is p: d/dt of ocean_surface_sample's V(p),
 * including the motion of the later cascades' sampling positions. xz holds points x 2 floats of base
 * points in device memory (for water above a world position: slots 0 and 2 of ocean_surface_query's
 * output). Per point, in unfused fp32, with GL_LINEAR + GL_REPEAT taps:
 *     px, pz = p;  py = 0;  ux = uy = uz = 0
 *     for c in cascades:           taps at (px / planeSize_c, pz / planeSize_c); s = displacement_c
 *         H, Dm = heightMap, displacementMap sample;  RH, RD = the two rate maps' samples
 *         vx = s * (RH.w + (Dm.y * ux + Dm.w * uz))       dDx/dt + grad Dx . u   (dDx/dz = Dm.w)
 *         vy =      RH.x + (H.y  * ux + H.z  * uz)        dh/dt  + grad h  . u
 *         vz = s * (RD.x + (Dm.w * ux + Dm.z * uz))       dDz/dt + grad Dz . u   (dDz/dx = dDx/dz)
 *         px += s * H.w;  py += H.x;  pz += s * Dm.x      exactly the vertex stage
 *         ux += vx;  uy += vy;  uz += vz
 *     out = (px, py, pz, 0,  ux, uy, uz, 0)
 * so slots 0-2 are ocean_surface_sample's bits; velocities in m/s. Argument rules, (generator,
 * cascade) rules and stream as ocean_surface_sample; no atlas. Every generator's rates must be
 * calculated and fresh: otherwise OCEAN_ERR_INVALID, naming the index of the generator in `gens`,
 * before any device call. points == 0 launches nothing. No reference counterpart. */
int ocean_surface_velocity(ocean_generator* const* gens, const int* cascades, int count, const float* xz,
                           int64_t points, float* out);

/* ---- Depth layers: water velocity and pressure head below the surface ---------------------------
 * The calls above describe the surface particle; a keel 3 m down, a mooring line, an ROV or an underwater
 * camera sits in water whose orbital motion has decayed, in deep water as e^{-kd} and in finite depth by
 * a cosh / sinh profile, differently for every wavenumber (more than a factor of 10 over 1 m for the 5 m
 * cascade, little for the 101 m one). The factor is per wavenumber, so it is applied in k space, before
 * the transform: a generator holds a short list of rest depths ("depth layers") and, per depth, two maps
 * per cascade with the water velocity and the pressure head under every texel.
 *
 * ocean_generator_set_depth_layers: `depths` is a host array of 1..8 floats, the rest depths in metres
 * below the mean water level: finite, >= 0 and strictly ascending, else OCEAN_ERR_INVALID. The list is
 * per generator and shared by its cascades. Setting it marks the layers stale; a change of the layer
 * count frees their storage after the generator's stream has drained. Whole-grid generators only.
 * ocean_generator_depth_layers returns the count (0: none set, or a null generator) and copies the
 * depths to `out` when it is not null.
 *
 * ocean_generator_calculate_kinematics: the rules of ocean_generator_calculate_rates (whole-grid
 * generators only, every N in 16 .. 16384, every frame path, after at least one frame, on the
 * generator's stream, no host synchronisation) and a depth list set. One launch of the packing kernel
 * (16 B read and 32 * layers B written per point), then one batched EncodeIFFT over the
 * 2 * layers * cascades images. The storage, [cascade][layer][2][N * N] RGBA32F, 32 B per point, cascade
 * and layer, is allocated on first use (OCEAN_ERR_OOM when that fails) and freed by
 * ocean_generator_destroy. The layers are fresh until the next frame call or the next
 * ocean_generator_set_depth_layers; the library tracks that on the host.
 *
 * Contract of the packed images, per cascade, texel and layer depth d, in fp32: k, w, the phase, g and h
 * are those of the last column pass, H the frame's evolved amplitude and Hd = dH/dt as in
 * ocean_generator_calculate_rates, and with dc = min(d, h)
 *     A_h = cosh(k (h - dc)) / cosh(k h),      A_v = sinh(k (h - dc)) / sinh(k h)   (0 when h == 0),
 * evaluated as  e1 = exp(-(k dc)), e2 = exp(-((2k)(h - dc))), e3 = exp(-((2k) h)),
 *     A_h = e1 * ((1 + e2) / (1 + e3)),        A_v = e1 * (expm1(-((2k)(h - dc))) / expm1(-((2k) h))),
 * which is exactly 1.0f for both at d == 0 (h > 0). The layers keep prepareFFT's own lanes
 * (spectrum.compute:236-237), each complex lane times a real factor:
 *     image 0 = ( A_v * lane xy of the height packing of Hd,        A_h * lane zw of the height packing of Hd )
 *     image 1 = ( A_h * lane xy of the displacement packing of Hd,  A_h * lane xy of the height packing of H )
 * A real multiple keeps a lane's (field, partner) structure, so the Nyquist-row defect of the reference's
 * spectrum is attenuated at its own wavenumber, and at d == 0 the lanes are those of the rate maps and of
 * the height map bit for bit. (A packing of the physical fields alone, (Dx + i eta, Dz + i P), differs
 * from what the library shows at the surface by 3 .. 50 % per channel because of that defect.) After
 * EncodeIFFT:
 *     image 0:  .x = vertical velocity in m/s,  .y = its x-slope,  .w = d/dt of Dx at depth
 *     image 1:  .x = d/dt of Dz at depth,  .z = pressure head in metres,  .w = its x-slope
 * and the other channels hold the frame's partner fields. Horizontal velocities are scale * d/dt (Dx, Dz),
 * as everywhere in the library. Both profiles are normalised to 1 at the surface: in finite depth that
 * follows the library's own surface, whose Dx / Dz carry no coth(k h), and not textbook linear theory,
 * whose horizontal profile is cosh(k (h - d)) / sinh(k h). At d >= h the vertical velocity is 0.
 * No reference counterpart. */
int ocean_generator_set_depth_layers(ocean_generator* gen, const float* depths, int layers);
int ocean_generator_depth_layers(const ocean_generator* gen, float out[8]);
int ocean_generator_calculate_kinematics(ocean_generator* gen);
/* RGBA32F N*N, row-major, holding what the last ocean_generator_calculate_kinematics wrote; valid until
 * the generator is destroyed or its layer count changes. Null, with ocean_last_error set, for a null
 * generator, a cascade out of range, layers that were never calculated, and a layer or image (0, 1) out
 * of range. */
float* ocean_generator_kinematics_map(ocean_generator* gen, int cascade, int layer, int image);
/* What the water is doing at world positions. xyz: points x 3 floats (X, Y, Z; Y up, 0 the mean water
 * level), out: points x 12 floats, both device memory. (generator, cascade) rules, argument rules and
 * stream as ocean_surface_query; no atlas. Every generator's layers must be calculated, fresh, and of a
 * depth list bit-identical to gens[0]'s: otherwise OCEAN_ERR_INVALID, naming the index of the generator in
 * `gens`, before any device call. points == 0 launches nothing.
 *
 * Per point, in unfused fp32, with D[0 .. L-1] the depths:
 *     Q = ocean_surface_query's vertex-stage fixed point at q = (X, Z):  p = (Q0, Q2), eta = Q1, res = Q7
 *     s = eta - Y;  wet = s > 0;  d = max(s, 0), NaN -> 0
 *     if   !(d > D[0])  : l = 0,     f = 0
 *     elif d >= D[L-1]  : l = L - 1, f = 0
 *     else l = largest index with D[l] <= d,  f = (d - D[l]) / (D[l+1] - D[l])
 *     px, pz = p;  ux = uy = uz = P = 0
 *     for c in cascades:      taps at (px / planeSize_c, pz / planeSize_c), GL_LINEAR + GL_REPEAT; sc = displacement_c
 *         a0, a1 = layer l's image 0 / 1 samples;  when f != 0: b0, b1 = layer l+1's, v = a + f * (b - a); else v = a
 *         ux += sc * v0.w;  uy += v0.x;  uz += sc * v1.x;  P += v1.z
 *         H, Dm = heightMap, displacementMap samples;  px += sc * H.w;  pz += sc * Dm.x     (the vertex stage's chain)
 *     out = (p.x, eta, p.z, res,   ux, uy, uz, P,   d, (float)l, f, wet ? 1 : 0)
 * Velocities in m/s, P the dynamic pressure head in metres of water. The rest depth of a point is taken
 * as its depth under the instantaneous surface (the deep-water limit of Wheeler stretching).
 * Approximations: the column under a surface particle is sampled at that particle's base point;
 * ocean_surface_velocity's grad . u terms are not carried below the surface; above the first layer and
 * below the last the nearest layer is held; the blend is linear in depth, so space the layers
 * geometrically. With D[0] = 0 a point at or above the water gets the surface particle's velocity without
 * the chain terms. No reference counterpart. */
int ocean_water_kinematics(ocean_generator* const* gens, const int* cascades, int count, const float* xyz,
                           int64_t points, int iterations, float tolerance, float* out);

/* ---- Bounds of the maps and ray casting against the displaced surface --------------------------
 * The calls above map base points and world positions to the water; these answer the line-of-sight
 * question, where a ray meets it (lidar / radar / camera sensor models, picking, impacts, "is the camera
 * under water along this ray"). A march needs the slab the surface lives in, so the bounds come first.
 *
 * ocean_generator_build_bounds enqueues, on the generator's stream, the minimum and maximum of every
 * channel of the current maps: per cascade 18 floats, for channel j of (heightMap.x, .y, .z, .w,
 * displacementMap.x, .y, .z, .w, jacobian) [2j] is the minimum and [2j + 1] the maximum over the N^2
 * texels. Exact values (any reduction order gives them; -0 and +0 compare equal); maps holding NaN are
 * unspecified. Two kernel launches, 36 B read per point, no host synchronisation, no float atomics. The
 * storage (the table and 72 B per 2048 texels of scratch) is allocated on the first call (OCEAN_ERR_OOM
 * when that fails) and freed by ocean_generator_destroy. Whole-grid generators only, every N in
 * 16 .. 16384: a slab generator and a generator that has calculated no frame yet get OCEAN_ERR_INVALID
 * before any device call. The bounds are fresh until the next call that rewrites the maps
 * (ocean_generator_calculate and the other frame calls); the library tracks that on the host.
 * Uses beside the ray march: culling boxes (heightMap.x, heightMap.w and displacementMap.x are h, Dx and
 * Dz), and min jacobian > 0 as the sign that ocean_surface_query's fixed point converges everywhere.
 * No reference counterpart. */
int ocean_generator_build_bounds(ocean_generator* gen);
/* Host copy of one cascade's 18 floats; synchronises the generator's stream. OCEAN_ERR_INVALID for a null
 * generator or output, a cascade out of range, and bounds that were never built or are stale. */
int ocean_generator_bounds(ocean_generator* gen, int cascade, float out[18]);
/* The table [cascade][18] in device memory, valid until the generator is destroyed. Null, with
 * ocean_last_error set, for a null generator and for bounds that were never built or are stale. */
const float* ocean_generator_bounds_device(ocean_generator* gen);
/* Where rays meet the water. rays: n_rays x 8 floats (ox, oy, oz, tmin, dx, dy, dz, tmax), out: n_rays x 16
 * floats, both device memory. (generator, cascade) rules and stream as ocean_surface_sample; no atlas.
 * Every generator's bounds must be built and fresh: otherwise OCEAN_ERR_INVALID, naming the index of the
 * generator in `gens`, before any device call.
 *
 * Contract, per ray, in unfused fp32. V(p) is ocean_surface_sample's vertex stage at base point p, the
 * fragment stage is its fragment stage; bounds_c is the row of pair c; min and max return NaN when either
 * operand is NaN.
 *   slab (read on the device from the bounds tables, no host synchronisation):
 *     ylo = 0; yhi = 0; for each pair c in order: ylo += bounds_c[0]; yhi += bounds_c[1]
 *     ylo -= pad; yhi += pad
 *   clip:
 *     t0 = tmin; t1 = tmax
 *     if dy == 0:  if !(ylo <= oy && oy <= yhi): OUTSIDE
 *     else: a = (ylo - oy) / dy; b = (yhi - oy) / dy; t0 = max(t0, min(a, b)); t1 = min(t1, max(a, b))
 *     if !(t0 <= t1): OUTSIDE                      (NaN lands here)
 *   one evaluation E(t), carrying the warm-start offset `off` (initially (0, 0)) from one to the next:
 *     q = (ox + t*dx, oz + t*dz);  p = q + off;  V = V(p)
 *     repeat at most `iterations` times:
 *         r = q - V.xz;  if max(|r.x|, |r.z|) <= tolerance: stop;  p = p + r;  V = V(p)
 *     off = p - q;  g = (oy + t*dy) - V.y
 *   march:
 *     inv = (slope == +inf) ? 0 : 1 / (|dy| + slope * sqrt(dx*dx + dz*dz))
 *     ta = t0; ga = E(ta); below = (ga <= 0); steps = 0
 *     loop: if steps == max_steps: STEP_LIMIT
 *           tb = min(ta + max(step, |ga| * inv), t1); gb = E(tb); steps += 1
 *           if (gb <= 0) != below: crossing found, leave the loop
 *           ta = tb; ga = gb; if tb >= t1: EXIT
 *   refine (crossings only), `refine` times:
 *     tm = 0.5f * (ta + tb); gm = E(tm); if (gm <= 0) == below: (ta, ga) = (tm, gm) else (tb, gb) = (tm, gm)
 *     then t = ta + (tb - ta) * (ga / (ga - gb))
 *   final: one more E(t) (for EXIT and STEP_LIMIT at t = ta), then the fragment stage at its V.xz
 *   out row 0: (ox + t*dx, oy + t*dy, oz + t*dz, t)
 *       row 1: (nx, ny, nz, jacobian)
 *       row 2: (p.x, V.y, p.z, max(|q.x - V.x|, |q.z - V.z|))      ocean_surface_query's slots 0, 1, 2, 7
 *       row 3: (status, below ? 1 : 0, steps, g of the final evaluation)
 *   status: 0 HIT, 1 OUTSIDE (rows 0-2 all zero, row 3 = (1, 0, 0, 0)), 2 EXIT, 3 STEP_LIMIT
 * t is in units of |d| (metres when d is normalised); `step` is the coarsest advance. `slope` is the
 * caller's bound on the slope of the surface: with it a ray far above the water advances by its clearance
 * |g| / (|dy| + slope * |d.xz|) instead of by `step`; +inf means fixed steps. The hit is the first sign
 * change ON THE MARCHED LATTICE: a crest thinner than the advance can be stepped over, and with a finite
 * slope the lattice depends on the clearances. A ray that starts under water (below = 1) hits from below.
 * The warm start makes the water height differ, within the tolerance, from composing ocean_surface_query
 * calls: that is deliberate, it is why an evaluation costs about one vertex stage. Every loop is bounded
 * by its count: rays with non-finite entries or a zero direction do not make the call fail, they follow
 * the arithmetic above, whatever it gives.
 * One kernel launch, one lane per ray; no host synchronisation, no allocation.
 * OCEAN_ERR_INVALID, before any device call: null gens / cascades; step not finite or <= 0; max_steps
 * outside 1..65535; refine outside 0..32; iterations outside 0..64; a negative or non-finite tolerance or
 * pad; slope negative or NaN; negative n_rays; null rays / out with n_rays > 0. n_rays == 0 launches
 * nothing. No reference counterpart. */
int ocean_surface_raycast(ocean_generator* const* gens, const int* cascades, int count, const float* rays,
                          int64_t n_rays, float step, int max_steps, int refine, int iterations, float tolerance,
                          float slope, float pad, float* out);

/* ---- Camera images: ray-cast pixels shaded with the reference's water, sky and fog ----------------
 * The last step of a camera model: one fused kernel, one lane per pixel, camera ray -> the march of
 * ocean_surface_raycast -> fragment stage (on the mip pyramid by the pixel's footprint when lod_scale > 0)
 * -> the water colour of resources/waveShader.glsl:146-160 -> the fog of :221-233 -> the sky of :41-63.
 * No rasteriser: the picture is what the rays see. Not reproduced: the reference's double 8-bit
 * quantisation (a BGRA8 framebuffer, then the post pass) and its finite warped mesh; here the water reaches
 * far_plane. The 45 degree field of view of ocean_default_camera is this library's choice (the reference's
 * value lives in its engine, not in its tree).
 *
 * ocean_camera: position and a world-space basis (viewInverse columns 0, 1 and -column 2); near_plane and
 * far_plane are depth planes as in the rasteriser; lod_scale 0 samples level 0 and needs no pyramid.
 * ocean_shading: WaveRenderData of the reference's src/Renderer.h, and the fog density of
 * waveShader.glsl:230. ocean_march: ocean_surface_raycast's parameters.
 *
 * Contract, per pixel (i, j) (row 0 is the top row, x fastest), in unfused fp32:
 *   ray:  aspect = (float)width / (float)height;  T = tan_half_fov_y
 *         x = (((2*(i + 0.5)) / (float)width) - 1) * (aspect * T)
 *         y = (1 - ((2*(j + 0.5)) / (float)height)) * T
 *         len = sqrt((x*x + y*y) + 1)
 *         d.k = ((x*right.k + y*up.k) + forward.k) / len
 *         ray = (position, near_plane*len, d, far_plane*len)       ocean_camera_rays writes exactly these
 *   march: ocean_surface_raycast's contract on that ray: status, t, the point V of the final evaluation
 *         and the fragment stage at V.xz; view depth z = t / len. With lod_scale > 0 the fragment stage is
 *         ocean_surface_sample_lod's at V.xz with footprint = lod_scale * (z * ((2*T) / (float)height)),
 *         the world size of a pixel at that depth; the march itself always runs on level 0.
 *   host constants, in double, rounded once: L = light_direction / |light_direction|,
 *         cthr = cos(sun_view_angle * 0.0174533), cfade = cos((sun_view_angle + max(sun_falloff_angle, 0.01))
 *         * 0.0174533)
 *   dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z;  normalize(v) = v / sqrt(dot(v, v));  min and max return NaN
 *         when either operand is NaN
 *   sky(v): u = normalize(v);  s = dot(L, u)
 *         e = min(max((s - cfade) / (cthr - cfade), 0), 1);  w = (e*e) * (3 - 2*e);  w = w * (w*w)
 *         m = 0.8 - u.y / 0.8;  m = m*m
 *         box.c = sky_color.c*(1 - m) + light_color.c*m
 *         sky.c = (1 - w)*box.c + (2*w)*light_color.c
 *   water (status 0 only; hits from below are shaded the same):
 *         n = the fragment stage's normal;  P = V;  I = -normalize(position - P)
 *         k = 2*dot(n, I);  r = I - k*n
 *         diffuse = max(dot(n, L), 0) * 0.3
 *         sp = max(dot(r, L), 0);  sp = sp*sp five times;  specular = sp * 0.5
 *         scatter = max(P.y * 0.1, 0);  light = (diffuse + 0.5) + specular
 *         col.c = ((light * wave_color.c) * sky(r).c) + scatter * scatter_color.c
 *         f = max(1 - expf(-((z - fog_begin) * fog_density)), 0)
 *         out.c = col.c*(1 - f) + sky(d).c*f
 *   every other status: out = sky(d)
 *   image = (out, 1);  aux = (t, z, the fragment stage's jacobian, status), OUTSIDE gives (0, 0, 0, 1)
 *   image8: per channel !(c > 0) ? 0 : (uint8)(min(c, 1)*255 + 0.5), alpha 255, RGBA order
 * image and aux are width*height x 4 floats, image8 width*height x 4 bytes, all device memory; any of them
 * may be null, not all. (generator, cascade) rules, stream and the freshness of the bounds as
 * ocean_surface_raycast; with lod_scale > 0 every generator's pyramid must be built and fresh, as
 * ocean_surface_sample_lod asks. One kernel launch (a 16 x 16 pixel tile per work item), no allocation, no
 * host synchronisation, no atomics: a call replays bit for bit.
 * OCEAN_ERR_INVALID, before any device call: null gens / cascades / camera / shading / march; width or
 * height outside 1..16384; a non-finite camera entry; tan_half_fov_y <= 0; near_plane < 0 or near_plane >=
 * far_plane; lod_scale negative or non-finite; a non-finite shading entry; a zero light_direction; a negative
 * sun_view_angle, sun_falloff_angle or fog_density; the march's rules as ocean_surface_raycast states them;
 * all three outputs null. */
typedef struct ocean_camera
{
  float position[3];
  float right[3], up[3], forward[3]; /* world-space basis: viewInverse columns 0, 1 and -column 2 */
  float tan_half_fov_y, near_plane, far_plane;
  float lod_scale; /* 0: level-0 sampling, no pyramid needed */
} ocean_camera;
typedef struct ocean_shading /* WaveRenderData of the reference's src/Renderer.h */
{
  float wave_color[3], scatter_color[3], sky_color[3], light_color[3], light_direction[3];
  float sun_view_angle, sun_falloff_angle, fog_begin, fog_density;
} ocean_shading;
typedef struct ocean_march
{
  float step;
  int max_steps, refine, iterations;
  float tolerance, slope, pad;
} ocean_march;
/* Position (0, 5, 0), pitch -5 and yaw -135 degrees, near 1, far 1500 (src/Renderer.cpp:14-16), with
 * forward = (cos p sin y, sin p, -cos p cos y), right = (cos y, 0, sin y), up = right x forward evaluated in
 * double and rounded once; a 45 degree vertical field of view; lod_scale 0. */
void ocean_default_camera(ocean_camera* camera);
/* src/Renderer.h:22-29 as written there, fog_density 0.0025 (waveShader.glsl:230). */
void ocean_default_shading(ocean_shading* shading);
/* step 0.25, 256 steps, 10 bisections, 4 iterations, tolerance 1e-3, slope 1, pad 0. */
void ocean_default_march(ocean_march* march);
/* The rays of the contract above: rays is width*height x 8 floats in device memory, enqueued on hip_stream
 * (a hipStream_t; null: the default stream). The camera's rules as ocean_camera_render; null rays refused. */
int ocean_camera_rays(const ocean_camera* camera, int width, int height, float* rays, void* hip_stream);
int ocean_camera_render(ocean_generator* const* gens, const int* cascades, int count, const ocean_camera* camera,
                        const ocean_shading* shading, const ocean_march* march, int width, int height, float* image,
                        float* aux, uint8_t* image8);

/* ---- Camera layers: whitecaps in the water pass, spray records splatted over it -----------------
 * ocean_camera_render with what makes a sea look white: the persistent foam (ocean_generator_advance_foam)
 * shaded under the fog, and spray records (an ocean_particles list, or an ocean_spray_emit call's out)
 * drawn as small screen-space sprites with a per-pixel depth test against the water each pixel's ray found,
 * a hit count and the nearest record's index. The same inputs give the same bytes on every run. No
 * reference counterpart (the reference draws neither); the defaults of ocean_default_camera_layers are
 * starting points, not measurements.
 *
 * Contract, in unfused fp32, with ocean_camera_render's names (T = tan_half_fov_y, aspect, dot, min, max,
 * sky, col, diffuse, z, V, d, f):
 *   water pass: ocean_camera_render's contract with one insertion at status 0 when foam_opacity > 0, after
 *         col and before the fog:
 *         foam = the persistent foam at V.xz: the sum over pairs of tap_c(F_c) / (float)count, accumulated
 *                as the fragment stage accumulates the Jacobian there (ocean_surface_sample_foam's slot 7 for
 *                a point displaced to V.xz); always on level 0, also with lod_scale > 0
 *         w = min(max((foam - foam_lo) / (foam_hi - foam_lo), 0), 1);  w = (w*w) * (3 - 2*w)
 *         w = w * foam_opacity
 *         fc.c = (diffuse + 0.5) * foam_color.c
 *         col'.c = col.c*(1 - w) + fc.c*w          then out.c = col'.c*(1 - f) + sky(d).c*f as before
 *         Every generator then needs foam storage (ocean_surface_sample_foam's rule).
 *   spray pass (records non-null and max_records > 0): n = min(*count_device, max_records) read on the
 *         device (a null count_device: n = max_records; a negative count: 0). For each record r < n with
 *         p = its slots 0..2:
 *         e = p - position;  z = dot(e, forward);  x = dot(e, right);  y = dot(e, up)
 *         culled unless z >= near_plane && z <= far_plane                           (NaN culls)
 *         sx = ((x / (z * (aspect*T))) + 1) * (0.5f * (float)width);   ci = floorf(sx)
 *         sy = (1 - (y / (z * T))) * (0.5f * (float)height);           cj = floorf(sy)
 *         half = (int)min(floorf(spray_radius / (z * ((2*T) / (float)height))), (float)spray_max_half),
 *                a NaN gives 0
 *         culled unless (float)-half <= ci <= (float)(width-1+half) and (float)-half <= cj <=
 *                (float)(height-1+half), compared in float                          (NaN culls)
 *         for every pixel q = (ci+a, cj+b), |a|, |b| <= half, inside the image:
 *             passes iff aux[q].status != 0 || z < aux[q].z          (the water pass's view depth)
 *             key[q] = min(key[q], (uint64)bits(z) << 32 | r);   hits[q] += 1
 *         key starts at all ones and hits at 0. A record that passes has z > 0 (z = 0 projects to infinity),
 *         so the bits of z order as the floats do; equal depths resolve to the lower record index. min and +
 *         are integer atomics: they commute, so the words do not depend on the order of arrival.
 *   composite, per pixel with c = hits > 0, zs = the key's high word as a float, r = its low word, base = the
 *         water pass's pixel:
 *         a = min((float)c * spray_opacity, 1)
 *         fs = max(1 - expf(-((zs - fog_begin) * fog_density)), 0)
 *         s.c = spray_color.c * light_color.c;   sc.c = s.c*(1 - fs) + sky(d).c*fs
 *         out.c = base.c*(1 - a) + sc.c*a
 *         c == 0: out = base.
 *   image = (out, 1);  image8 from out as ocean_camera_render's;  aux = the water pass's, unchanged
 *   aux2 = (foam, zs, the bits of the uint32 c, the bits of the uint32 r): foam is 0 where status != 0 or
 *         foam_opacity == 0; a pixel without spray has zs = 0, c = 0, r = 0xFFFFFFFF.
 * image, aux, aux2: width*height x 4 floats; image8: width*height x 4 bytes; device memory, any of them null,
 * not all. records: device memory, 8 floats per record, 4-byte aligned. scratch: caller-owned device memory
 * of ocean_camera_layers_scratch_bytes(width, height) bytes (48 per pixel and at most 32 of padding; 0 for a
 * width or height outside 1..16384), 16-byte aligned, needed only when the spray pass runs: the per-pixel
 * key, hit count and foam, and the float image and aux where the caller passed null for them. Its contents
 * are undefined after the call.
 * With foam_opacity == 0 and no spray pass the picture is ocean_camera_render's own launch (the same kernel),
 * and aux2, if asked for, a constant fill in a launch of its own. With foam and no spray: one launch. With
 * spray: three (water, splat, composite). All on the plan's stream under its CU budget; no allocation, no
 * host synchronisation.
 * OCEAN_ERR_INVALID, before any device call: everything ocean_camera_render refuses (up to its outputs);
 * null layers; a non-finite layers entry; foam_lo >= foam_hi; foam_opacity or spray_opacity outside 0..1;
 * a negative spray_radius; spray_max_half outside 0..8; max_records outside 0..2^28; records non-null with
 * max_records > 0 and a null scratch; all four outputs null. Then the generators' rules as
 * ocean_camera_render, and with foam_opacity > 0 a generator without foam storage (named by its index). */
typedef struct ocean_camera_layers
{
  float foam_color[3];    /* default (1, 1, 1) */
  float foam_lo, foam_hi; /* foam value where whitecaps begin / are full; default 0.25, 0.75 */
  float foam_opacity;     /* 0: no foam stage, no foam storage needed; default 1 */
  float spray_color[3];   /* default (1, 1, 1) */
  float spray_radius;     /* metres: world half-size of a particle's sprite; default 0.05 */
  int32_t spray_max_half; /* sprite half-size cap in pixels, 0..8; default 2 */
  float spray_opacity;    /* per particle covering a pixel; default 0.25 */
} ocean_camera_layers;
void ocean_default_camera_layers(ocean_camera_layers* layers);
size_t ocean_camera_layers_scratch_bytes(int width, int height);
int ocean_camera_render_layers(ocean_generator* const* gens, const int* cascades, int count,
                               const ocean_camera* camera, const ocean_shading* shading, const ocean_march* march,
                               const ocean_camera_layers* layers, int width, int height, const float* records,
                               const int64_t* count_device, int64_t max_records, void* scratch, float* image,
                               float* aux, float* aux2, uint8_t* image8);

/* ---- Hull sets: net wave force and torque on batches of floating bodies -------------------------
 * The consumer of the three sections above: a floating body is a set of hull points, each carrying a
 * displaced volume and drag coefficients; per step the caller hands in the bodies' poses and gets one
 * wrench (force and torque about the body's centre) per body back. One fused pass: pose -> world point ->
 * ocean_surface_query -> ocean_surface_velocity -> load -> sum per body, with no intermediate in device
 * memory, and a summation order that is part of the contract, so a step is replayable bit for bit.
 *
 * ocean_hulls_create. points: host, n_points x 8 floats (lx, ly, lz, volume, half_height, drag_lin,
 * drag_quad, 0) in the body frame. ranges: host, bodies x 2 int32 (first, count) into points; bodies may
 * share or overlap ranges (instances of one hull). Both are copied to the device of `fft` (the current
 * device); later calls run on its stream. Also built here: the table of work items (64-point tiles of one
 * body) and the scratch for the partial sums of bodies of more than 64 points.
 * OCEAN_ERR_INVALID, before any device call: null out / fft / points / ranges; bodies outside
 * 1 .. 1048576; a count outside 1 .. 262144 or a range that leaves points; a non-finite point field;
 * volume < 0, half_height <= 0 or a negative drag coefficient. */
typedef struct ocean_hulls ocean_hulls;
int ocean_hulls_create(ocean_hulls** out, ocean_fft* fft, const float* points, int64_t n_points,
                       const int32_t* ranges, int bodies);
/* Waits for the plan's stream, then frees the set. */
int ocean_hulls_destroy(ocean_hulls* hulls);
int ocean_hulls_bodies(const ocean_hulls* hulls);
int64_t ocean_hulls_instance_points(const ocean_hulls* hulls);   /* sum of the counts */
/* poses: device, bodies x 20 floats (R[9] row-major body->world, c[3], v[3], w[3], 0, 0): rotation,
 * centre, linear and angular velocity in the world frame. loads: device, bodies x 8 floats.
 * point_out: device, instance_points x 8 floats, or null.
 *
 * Contract, in unfused fp32. For body b with range (first, cnt) and point i < cnt, L = points[first + i],
 * and R, c, v, w from poses[b]:
 *     d   = (R0*L.x + R1*L.y) + R2*L.z,  (R3*L.x + R4*L.y) + R5*L.z,  (R6*L.x + R7*L.y) + R8*L.z
 *     x   = c + d
 *     Q   = ocean_surface_query at q = (x.x, x.z) with (iterations, tolerance):
 *           base p = (Q0, Q2), eta = Q1, res = Q7
 *     t   = (eta - x.y) / (L.half_height + L.half_height) + 0.5f
 *     s   = min(max(t, 0), 1), NaN t -> 0                       submerged fraction
 *     u   = slots 4..6 of ocean_surface_velocity at base p when water_velocity, else 0
 *     vp  = v + (w.y*d.z - w.z*d.y, w.z*d.x - w.x*d.z, w.x*d.y - w.y*d.x)
 *     rel = u - vp;   m = sqrtf((rel.x*rel.x + rel.y*rel.y) + rel.z*rel.z)
 *     k   = s * (L.drag_lin + L.drag_quad * m)
 *     F   = (k*rel.x,  rho_g * (L.volume * s) + k*rel.y,  k*rel.z)
 *     T   = (d.y*F.z - d.z*F.y,  d.z*F.x - d.x*F.z,  d.x*F.y - d.y*F.x)      torque about c
 *     a_i = (F.x, F.y, F.z, L.volume*s,  T.x, T.y, T.z, s > 0 ? 1 : 0)
 *     point_out[offset_b + i] = (p.x, eta, p.z, res,  F.x, F.y, F.z, s)      offset_b = sum of earlier counts
 * Only the query's vertex stage is evaluated (the normal and the Jacobian are not used). So loads[b] is
 * (force, submerged volume, torque about the centre, number of wet points): the sum of a_i, component by
 * component, in this fixed order, which is part of the contract:
 *     fold64(a): pad a (len <= 64) with +0.0f to 64; for h in 32,16,8,4,2,1: a = a[:h] + a[h:]; return a[0]
 *     sum(a):    len <= 64 -> fold64(a); else sum([fold64(a[j:j+64]) for j in 0,64,128,...])
 * a radix-64 tree over consecutive points. No float atomics: the same poses on the same maps give the same
 * bits on every run and for every split of the bodies over calls. One freedom is taken: consecutive bodies
 * of at most 32 points share a wave in aligned power-of-two segments and skip the fold steps that would add
 * the +0.0f padding, so a sum that is zero may carry either sign.
 *
 * At most two kernel launches on the plan's stream (the second only when a body has more than 64 points),
 * plus the atlas repack where ocean_surface_query's rule would use it for instance_points points (the same
 * bits either way; the plan's atlas grows on first use as there). No host synchronisation, and no other
 * allocation after create.
 * OCEAN_ERR_INVALID, before any device call: a null hull set; the argument rules of ocean_surface_query
 * (iterations 0..64, tolerance finite and >= 0, its (generator, cascade) rules); a non-finite or negative
 * rho_g; null poses or loads; gens[0] on a plan other than the hull set's; water_velocity other than 0 or
 * 1; water_velocity == 1 with rates that were never calculated or are stale (the rule of
 * ocean_surface_velocity, naming the index in `gens`). With water_velocity == 0 the water is taken at
 * rest and rates are not needed. No reference counterpart. */
int ocean_hulls_loads(ocean_hulls* hulls, ocean_generator* const* gens, const int* cascades, int count,
                      const float* poses, float rho_g, int iterations, float tolerance, int water_velocity,
                      float* loads, float* point_out);

/* ---- Hull dynamics: bodies stepped on the device from their wave loads ---------------------------
 * ocean_hulls_loads gives a wrench per body; ocean_hulls_step also moves the bodies with it, so that
 * boats, buoys and debris float without leaving the device: rigid bodies with a diagonal inertia, integrated
 * by semi-implicit Euler in substeps, the loads evaluated anew at every substep's pose. The water is frozen
 * during a call and the bodies do not interact. Like the loads the step is unfused fp32 in a fixed order, so
 * a run replays bit for bit.
 *
 * ocean_hulls_set_bodies. props: host, bodies x 8 floats (mass, Ix, Iy, Iz, lin_damp, ang_damp, kinematic,
 * 0): the principal moments of inertia (the principal axes are the body-frame axes), linear and angular
 * damping in 1/s, and kinematic = 1 for a body that keeps its velocities (moved by the caller, loaded by the
 * water) or 0 for a dynamic one. Copied to the set's device; the only allocation of the dynamics, made by
 * the first call (the step keeps its sums on chip and needs no buffer for a caller that passes no loads).
 * A later call replaces the properties after waiting for the plan's stream.
 * OCEAN_ERR_INVALID, before any device call: a null argument; a non-finite field; mass or a moment <= 0; a
 * negative damping; kinematic other than 0 or 1. */
int ocean_hulls_set_bodies(ocean_hulls* hulls, const float* props);

typedef struct ocean_hull_step_settings {
  float dt; int32_t substeps;        /* dt finite > 0; substeps 1..64 */
  float gravity[3];                  /* default (0, -9.8, 0) */
  float rho_g; int32_t iterations; float tolerance; int32_t water_velocity;  /* as ocean_hulls_loads */
} ocean_hull_step_settings;
/* dt 1/60, substeps 1, gravity (0, -9.8, 0), rho_g 9810, iterations 8, tolerance 0, water_velocity 0 */
void ocean_default_hull_step_settings(ocean_hull_step_settings* settings);

/* poses: device, bodies x 20 floats in the layout of ocean_hulls_loads, updated in place. wrench_ext: device,
 * bodies x 8 floats or null: an external force in slots 0..2 and a torque about the centre in slots 4..6,
 * both in the world frame (thrust, mooring, towing); slots 3 and 7 are not read. loads (bodies x 8) and
 * point_out (instance_points x 8): device or null; they receive what ocean_hulls_loads returns for the pose
 * at the start of the last substep.
 *
 * Contract, in unfused fp32, every expression in the order written. h = dt / (float)substeps, computed on the
 * host. Per substep and body, with R (row-major, R[i][j] = slot 3i + j), c, v, w from the pose, (mass, I,
 * lin_damp, ang_damp, kinematic) from its properties, E its wrench_ext row and g = gravity:
 *     Lb  = the ocean_hulls_loads result for this pose: the same arithmetic, fold64 tree and bits
 *     F   = Lb[0..2] + E[0..2],  T = Lb[4..6] + E[4..6]      wrench_ext null: F = Lb[0..2], T = Lb[4..6]
 *   dynamic body (kinematic == 0), for k = x, y, z:
 *     v'.k  = (v.k + h * (F.k / mass + g.k)) / (1.0f + h * lin_damp)
 *     wb.k  = (R[0][k]*w.x + R[1][k]*w.y) + R[2][k]*w.z              wb = R^T w, the spin in the body frame
 *     Tb.k  = (R[0][k]*T.x + R[1][k]*T.y) + R[2][k]*T.z
 *     L     = (I.x*wb.x, I.y*wb.y, I.z*wb.z)
 *     G     = (wb.y*L.z - wb.z*L.y,  wb.z*L.x - wb.x*L.z,  wb.x*L.y - wb.y*L.x)
 *     wb'.k = (wb.k + h * ((Tb.k - G.k) / I.k)) / (1.0f + h * ang_damp)
 *     w'.k  = (R[k][0]*wb'.x + R[k][1]*wb'.y) + R[k][2]*wb'.z
 *   kinematic body: v' = v, w' = w
 *   both kinds:
 *     c'.k  = c.k + h * v'.k
 *     a     = ((0.5f*h)*w'.x, (0.5f*h)*w'.y, (0.5f*h)*w'.z);   n = (a.x*a.x + a.y*a.y) + a.z*a.z
 *     p = 1.0f - n;  q = 1.0f + n                    the Cayley map Q = ((1 - n) I + 2 a a^T + 2 [a]x) / (1 + n)
 *     Q[0][0] = (p + 2.0f*(a.x*a.x)) / q    Q[0][1] = (2.0f*(a.x*a.y) - 2.0f*a.z) / q    Q[0][2] = (2.0f*(a.x*a.z) + 2.0f*a.y) / q
 *     Q[1][0] = (2.0f*(a.x*a.y) + 2.0f*a.z) / q    Q[1][1] = (p + 2.0f*(a.y*a.y)) / q    Q[1][2] = (2.0f*(a.y*a.z) - 2.0f*a.x) / q
 *     Q[2][0] = (2.0f*(a.x*a.z) - 2.0f*a.y) / q    Q[2][1] = (2.0f*(a.y*a.z) + 2.0f*a.x) / q    Q[2][2] = (p + 2.0f*(a.z*a.z)) / q
 *     R1[i][j] = (Q[i][0]*R[0][j] + Q[i][1]*R[1][j]) + Q[i][2]*R[2][j]
 *   one Gram-Schmidt pass over the rows r0, r1 of R1:
 *     l0 = sqrtf((r0.x*r0.x + r0.y*r0.y) + r0.z*r0.z);   e0 = r0 / l0
 *     d  = (e0.x*r1.x + e0.y*r1.y) + e0.z*r1.z;          u = r1 - d*e0     (u.k = r1.k - d*e0.k)
 *     l1 = sqrtf((u.x*u.x + u.y*u.y) + u.z*u.z);         e1 = u / l1
 *     e2 = (e0.y*e1.z - e0.z*e1.y,  e0.z*e1.x - e0.x*e1.z,  e0.x*e1.y - e0.y*e1.x)
 *   the new pose: rows e0, e1, e2, then c', v', w', and slots 18 and 19 written as 0.
 * No transcendental: sqrtf and the divisions are correctly rounded in this build, as the loads contract
 * relies on, so a float32 restatement agrees to the bit (tests/hull_step_ref.py). A rotation about a fixed
 * axis turns by 2 atan(h |w| / 2) per substep. The gyroscopic term G is explicit: a fast spin about a
 * non-principal direction gains energy unless it is resolved by substeps or held by ang_damp.
 *
 * Launches, on the plan's stream, with no host synchronisation and no allocation, on top of the atlas repack
 * under the rule of ocean_hulls_loads. Every body of at most 64 points: one launch for the whole call,
 * whatever substeps is; a body's pose stays in the registers of its wave, or its segment of a wave, across
 * the substeps. Otherwise two launches per substep: bodies of one tile integrate in the first, bodies of
 * several tiles in the second, after their last fold. Only the owner of a body writes its pose, and the tiles
 * of a larger body read it in the launch before the one that writes it, so the update in place is safe.
 * OCEAN_ERR_INVALID, before any device call: a null hull set, settings or poses; dt not finite or <= 0;
 * substeps outside 1..64; a non-finite gravity; everything ocean_hulls_loads rejects (but loads may be
 * null); properties that were never set. No reference counterpart. */
int ocean_hulls_step(ocean_hulls* hulls, ocean_generator* const* gens, const int* cascades, int count,
                     const ocean_hull_step_settings* settings, float* poses, const float* wrench_ext,
                     float* loads, float* point_out);

/* Debug: hull sets created after enable = 0 give every body its own waves; by default consecutive bodies
 * of at most 32 points share a wave (the same bits either way; tools/hulls_bench.py times both). */
int ocean_debug_hulls_packing(int enable);

/* ---- Mooring lines: cable chains stepped on the device, wrenches for hulls --------------------------
 * What produces ocean_hulls_step's wrench_ext for a moored body (a buoy, a barge, a fish-farm cage): every
 * line is a chain of 2 .. 64 lumped nodes joined by springs that carry tension only, hanging in the water of
 * ocean_water_kinematics (or in still water), resting on a flat bed, between an anchor fixed in the world and
 * a fairlead fixed in the frame of a body. One call steps every line through all its substeps in one kernel,
 * the line's state held on chip in between, and sums the lines' pulls into one wrench per body. Unfused fp32
 * in a fixed order, so a run replays bit for bit, and a numpy float32 restatement agrees to the bit
 * (tests/moorings_ref.py).
 *
 * ocean_moorings_create. lines: host, n_lines x 16 floats
 *     0..2 anchor A (world)    3..5 fairlead Lf (body frame; world when the line has no body)
 *     6 length (unstretched, > 0)    7 EA (> 0, N)    8 CA (internal damping, >= 0, N s)
 *     9 mass_per_m (> 0)    10 volume_per_m (>= 0)    11 drag_lin per metre (>= 0)    12 drag_quad per metre (>= 0)
 *     13..15 zero
 * attach: host, n_lines x 2 int32 (body, nodes): body in -1 .. bodies - 1, -1 for a line with both ends fixed
 * in the world; nodes in 2 .. 64, both ends counted. The host builds, in fp32, the per-line constants
 *     l0 = length / (float)(nodes - 1)
 *     mn = mass_per_m * l0,  vn = volume_per_m * l0,  dl = drag_lin * l0,  dq = drag_quad * l0     (per node)
 * the table of work items (one wave per item, one lane per node; consecutive lines of at most 32 nodes share
 * a wave in aligned power-of-two segments, the packing of the hull sets, which ocean_debug_hulls_packing
 * switches for mooring sets created after it too) and a CSR of the lines of each body in ascending line
 * index, and copies them to the device of `fft` with the storage of the nodes (32 B per node) and 16 B per
 * line; later calls run on its stream and allocate nothing.
 * OCEAN_ERR_INVALID, before any device call: a null out / fft / lines / attach; n_lines outside 1 .. 1048576;
 * bodies outside 0 .. 1048576; a body or a node count out of range; a non-finite field; a sign rule above
 * broken or a slot 13..15 that is not zero. */
typedef struct ocean_moorings ocean_moorings;
int ocean_moorings_create(ocean_moorings** out, ocean_fft* fft, const float* lines, const int32_t* attach,
                          int n_lines, int bodies);
/* Waits for the plan's stream, then frees the set. */
int ocean_moorings_destroy(ocean_moorings* moorings);
int ocean_moorings_lines(const ocean_moorings* moorings);
int64_t ocean_moorings_total_nodes(const ocean_moorings* moorings);   /* sum of the node counts */
/* The nodes: device, total_nodes x 8 floats, the lines' nodes one after another from the anchor to the
 * fairlead, rows (x, y, z, T, vx, vy, vz, flags): T the tension of the segment from this node to the next in
 * the last substep (0 in a line's last node), flags = 1 * wet + 2 * on_bed of the last substep (0 in the end
 * nodes, which have no water state). The caller may read and write them between calls on the plan's stream
 * (a checkpoint, a pre-laid catenary); a step reads x, y, z and vx, vy, vz of the interior nodes only. Asking
 * for the pointer counts as writing the nodes. Null for a null set. */
float* ocean_moorings_nodes(ocean_moorings* moorings);
/* One launch: every line's nodes on the straight segment from A to the fairlead's world position P (below),
 * node i at  A.k + ((float)i / (float)(nodes - 1)) * (P.k - A.k),  velocities, T and flags 0. poses: device,
 * bodies x 20 floats in the layout of ocean_hulls_loads; null only when no line has a body, else
 * OCEAN_ERR_INVALID (and for a null set). */
int ocean_moorings_reset(ocean_moorings* moorings, const float* poses);

typedef struct ocean_mooring_settings {
  float dt; int32_t substeps;        /* dt finite > 0; substeps 1..256 */
  float gravity[3];                  /* finite */
  float rho_g;                       /* finite, >= 0 */
  int32_t iterations; float tolerance;  /* as ocean_water_kinematics; read when water == 1 */
  int32_t water;                     /* 0: still water (eta = 0, u = 0); 1: ocean_water_kinematics at the node */
  float bed_y;                       /* the flat bed's height, finite */
  float bed_k, bed_c;                /* the bed's stiffness and damping per metre of line, >= 0 */
} ocean_mooring_settings;
/* dt 1/60, substeps 8, gravity (0, -9.8, 0), rho_g 9810, iterations 4, tolerance 0, water 0, bed_y -100,
 * bed_k 1e5, bed_c 1e3. A null pointer is ignored. */
void ocean_default_mooring_settings(ocean_mooring_settings* settings);

/* Steps the nodes in place by settings.dt in settings.substeps substeps. poses: device, bodies x 20 floats,
 * read once: the fairleads are frozen during a call (null only when no line has a body). wrench_ext: device,
 * bodies x 8 floats, every row overwritten, in ocean_hulls_step's layout so that it can be passed straight
 * on; null only when bodies == 0. line_out: device, n_lines x 8 floats, or null.
 *
 * Contract, in unfused fp32, every expression in the order written. h = dt / (float)substeps, computed on the
 * host; g = gravity; kb = bed_k * l0, cb = bed_c * l0. Per line with n nodes on body b:
 *   the fairlead, with R, c, v, w from poses[b], the expressions of ocean_hulls_loads:
 *     d   = (R0*Lf.x + R1*Lf.y) + R2*Lf.z,  (R3*Lf.x + R4*Lf.y) + R5*Lf.z,  (R6*Lf.x + R7*Lf.y) + R8*Lf.z
 *     P   = c + d;    vp = v + (w.y*d.z - w.z*d.y, w.z*d.x - w.x*d.z, w.x*d.y - w.y*d.x)
 *     b == -1:  d = 0, P = Lf, vp = 0
 *   node 0 is held at A with velocity 0 and node n-1 at P with velocity vp, whatever their rows hold.
 *   Per substep, from the nodes' x and v at its start:
 *   every segment j = 0 .. n-2, between nodes j and j+1:
 *     dv    = x[j+1] - x[j];   len = sqrtf((dv.x*dv.x + dv.y*dv.y) + dv.z*dv.z)
 *     e.k   = len > 0 ? dv.k / len : 0
 *     strain = (len - l0) / l0
 *     rate  = (((v[j+1].x - v[j].x)*e.x + (v[j+1].y - v[j].y)*e.y) + (v[j+1].z - v[j].z)*e.z) / l0
 *     t     = EA*strain + CA*rate;   T[j] = t > 0 ? t : 0        no compression; NaN -> 0
 *     S[j].k = T[j] * e.k
 *   every interior node i = 1 .. n-2:
 *     water == 1:  eta, u, wet = slots 1, 4..6 and 11 of ocean_water_kinematics at (x, y, z): the same
 *                  arithmetic, the same bits;    water == 0:  u = 0,  wet = (0.0f - y) > 0
 *     rel   = u - v;   m = sqrtf((rel.x*rel.x + rel.y*rel.y) + rel.z*rel.z)
 *     k     = wet ? dl + dq*m : 0
 *     F.k   = ((S[i].k - S[i-1].k) + k*rel.k) + mn*g.k
 *     wet:       F.y = F.y + rho_g*vn
 *     pen   = bed_y - y;   pen > 0:   F.y = F.y + kb*pen;   then F.k = F.k - cb*v.k for k = x, y, z;   on_bed
 *     v'.k  = v.k + h*(F.k / mn);    x'.k = x.k + h*v'.k
 *   the fairlead: Ff = -S[n-2] is summed over the substeps, sum.k = sum.k + (-S[n-2].k) from +0.0f; after the
 *   last substep Fm.k = sum.k / (float)substeps. The mean, so that the impulse dt * Fm handed to the hull is the
 *   one the line received over the call.
 * line_out row: (Fm.x, Fm.y, Fm.z, T[n-2] of the last substep, T[0] of the last substep, the exact maximum of
 * T over the line's segments in the last substep, the number of nodes on the bed, the number of wet nodes,
 * both of the last substep, as floats).
 * wrench_ext row of body b: (F, the number of its lines as a float, Tq, 0) with, over the body's lines in
 * ascending line index from +0.0f,  F.k = F.k + Fm.k  and  Tq = Tq + (d.y*Fm.z - d.z*Fm.y, d.z*Fm.x - d.x*Fm.z,
 * d.x*Fm.y - d.y*Fm.x), the torque about the centre in the hull contract's order; a body without a line gets
 * zeros.
 * No transcendental outside the water query: sqrtf and the divisions are correctly rounded.
 *
 * The scheme is explicit (semi-implicit Euler per node), so the axial mode of a line bounds the substep:
 *     h < l0 * sqrt(mass_per_m / EA)
 * (a steel chain of EA = 1e8 N and 100 kg/m in 2 m segments: h < 2 ms); past it the tensions grow without
 * bound. This is why substeps go to 256, four times ocean_hulls_step's. CA damps the axial mode.
 *
 * Two launches on the plan's stream whatever substeps is, the lines' and the per-body sum's (one when
 * bodies == 0); a line's positions, velocities and fairlead sum stay in the registers of its wave, or its
 * segment of a wave, across the substeps. No atomics, no host synchronisation, no allocation.
 * OCEAN_ERR_INVALID, before any device call: a null set or settings; dt not finite or <= 0; substeps outside
 * 1..256; a non-finite gravity or bed_y; rho_g, bed_k or bed_c negative or not finite; water other than 0 or
 * 1; iterations or tolerance outside ocean_water_kinematics' ranges; null poses while a line has a body; a
 * null wrench_ext while bodies > 0; nodes that were never reset nor written by the caller
 * (ocean_moorings_nodes). With water == 1 also everything else ocean_water_kinematics rejects (the
 * (generator, cascade) rules; depth layers that are not set, calculated,
 * fresh and identical across gens, naming the index in `gens`) and gens[0] on another plan than the set's.
 * With water == 0 no generator is needed: gens, cascades and count are not read and count may be 0.
 * Not modelled: bending stiffness, contact between lines or with hulls, bed friction beyond bed_c, lines
 * of more than 64 nodes. No reference counterpart. */
int ocean_moorings_step(ocean_moorings* moorings, ocean_generator* const* gens, const int* cascades, int count,
                        const ocean_mooring_settings* settings, const float* poses, float* wrench_ext,
                        float* line_out);

/* ---- Wake windows: hull loads drive local surface waves on the device -------------------------------
 * No reference counterpart (the reference has no bodies). Every section above freezes the water during a call:
 * the water pushes the hulls and nothing pushes back. A wake window adds that state as a separate, linear
 * layer on top of the ambient ocean: a square height field h in base-point space (the space of the maps and
 * of the persistent foam), stepped with Tessendorf's local deep-water operator ("Interactive Water Surfaces"),
 *     h_tt = -(g / dx) G * (h + P),
 * G a 13 x 13 convolution whose symbol approximates |k|, and forced by the vertical loads that
 * ocean_hulls_loads / ocean_hulls_step write to point_out: the hull's vertical load on the water is a surface
 * pressure, which the dynamic boundary condition turns into a head P added to h under the operator. A body at
 * rest makes the depression Archimedes asks for (h = -P is the fixed point), a moving body a Kelvin-type wake.
 * The caller adds ocean_wake_sample's values to what ocean_surface_query returns (linear superposition);
 * the ambient surface, the hull loads, the ray cast and the camera do not read a window.
 *
 * ocean_wake_create. size = M, a multiple of 16 in 32..4096; dx (m) finite and > 0; a finite origin;
 * smoothing = sigma in 0.3..0.55, 0 standing for the default 0.5. Texel (i, j), i along x and fastest (index
 * j * M + i), sits at the base point (ox + i * dx, oz + j * dx) with ox = origin_x + (float)off_i * dx and oz
 * likewise; the integer offsets off_i, off_j are changed only by ocean_wake_shift, so repeated shifts do not
 * drift. Storage: h and h_prev (4 B each) and one signed 64-bit accumulator A per texel, 16 B per texel,
 * allocated and zeroed at create (OCEAN_ERR_OOM when that fails); no later call allocates. Every call runs on
 * the stream of `fft` under its CU budget with no host synchronisation.
 * The taps are built on the host in double, before any device call, and rounded once to float:
 *     T[a][b] = (1 / 2 pi) int_0^inf q^2 exp(-sigma q^2) J0(q sqrt(a^2 + b^2)) dq,   0 <= a, b <= 6
 *             = sqrt(pi) / (4 sigma^1.5) exp(-x / 2) ((1 - x) I0(x / 2) + x I1(x / 2)) / (2 pi),  x = r^2 / (4 sigma).
 * The symbol of the truncated operator, the double cosine sum of the float taps, is evaluated on 257^2 points
 * of [-pi, pi]^2 and a sigma whose minimum is not > 0 is refused: a negative symbol is a growing mode (0.3 ..
 * 0.55 pass, minimum 1.3e-4 at 0.55; 0.6 fails). The operator is exact only for wavelengths well inside its
 * 13-texel support: its symbol at k = 0 is about 0.14 instead of 0 (the dropped r^-3 tail), so waves longer
 * than about 30 texels travel too fast (the table in DESIGN.md).
 * OCEAN_ERR_INVALID, naming the field: a null out or fft, and each rule above.
 *
 * ocean_wake_step. records: device, rows of 8 floats in the layout of point_out: slot 0 = x and slot 2 = z of
 * the base point, slot 5 = F.y, the water's vertical force on the point (N); a caller may fabricate rows (a
 * pressure source, a dropped object). n = min(*count_device, max_records), read on the device; a null
 * count_device gives n = max_records, a negative count 0. max_records in 0..2^28; null records with
 * max_records == 0 is a free step.
 * Contract, in unfused fp32, every expression in the order written. Host constants, with s = *settings:
 *     hs = s.dt / (float)s.substeps      c = ((hs * hs) * s.gravity) / dx
 *     hb = 0.5f * hs                     inv = 1.0f / ((s.rho_g * dx) * dx)
 * Splat, per record r < n with (x, z, F):
 *     m = F * inv;   u = (x - ox) / dx;   v = (z - oz) / dx
 *     culled unless u >= -1 && u < (float)M && v >= -1 && v < (float)M        (a NaN culls)
 *     i0 = floorf(u), fx = u - i0, and likewise j0, fz
 *     taps (i0, j0), (i0+1, j0), (i0, j0+1), (i0+1, j0+1), weights (1-fx)*(1-fz), fx*(1-fz), (1-fx)*fz, fx*fz;
 *     a tap whose index leaves 0..M-1 is dropped; for each kept tap t
 *     p = m * w;   p' = (p == p) ? min(max(p, -1048576.0f), 1048576.0f) : 0
 *     A[t] += (int64)(p' * 1048576.0f)             truncating toward zero; a no-return 64-bit integer atomic
 * Integer adds commute, so the words do not depend on the order of the list. P[t] = (float)A[t] * 0x1p-20f is
 * held fixed for the whole call.
 * Substep, s.substeps times, for every texel t = (i, j), from h and h_prev at its start:
 *     e[t] = h[t] + P[t], and 0 outside the window
 *     d = (float)min(i, j, M-1-i, M-1-j)
 *     r = s.border > 0 ? max((float)s.border - d, 0) / (float)s.border : 0
 *     alpha = s.damp + s.edge_damp * (r * r);   b = hb * alpha
 *     acc = +0.0f; then for a = 0..6 and b' = 0..a in that order acc = acc + T[a][b'] * S with
 *       (0, 0):      S = e[i, j]
 *       (a, 0):      S = (e[i+a, j] + e[i-a, j]) + (e[i, j+a] + e[i, j-a])
 *       (a, a):      S = (e[i+a, j+a] + e[i-a, j-a]) + (e[i+a, j-a] + e[i-a, j+a])
 *       0 < b' < a:  S = ((e[i+a, j+b'] + e[i-a, j-b']) + (e[i+a, j-b'] + e[i-a, j+b']))
 *                      + ((e[i+b', j+a] + e[i-b', j-a]) + (e[i+b', j-a] + e[i-b', j+a]))
 *     h_new[t] = (((2.0f * h[t]) - (1.0f - b) * h_prev[t]) - c * acc) / (1.0f + b)
 *     then h_prev = h and h = h_new.
 * The damping acts on the velocity, and the centred form has h = -P as its fixed point (Tessendorf's printed
 * form pulls the height to zero and does not). After the call every A[t] is 0 again.
 * Launches: at most substeps + 2: the splat (skipped when max_records == 0), one per substep (the 6-texel halo
 * makes a substep a global dependency) and one that zeroes the accumulators the splat touched.
 * Stability: with sum|T| over all 169 float taps in double, ocean_wake_max_substep returns
 * 2 sqrt(dx / (gravity sum|T|)) (0.29 s at dx = 0.25, sigma = 0.5; 0 for a null wake or a gravity that is not
 * > 0), and ocean_wake_step refuses hs at or above it. The bound is sufficient, not tight: the true limit is
 * about sqrt(2) higher.
 * OCEAN_ERR_INVALID, before any device call, naming the field: a null wake or settings; dt not finite or <= 0;
 * substeps outside 1..64; gravity or rho_g not finite or <= 0; a negative or non-finite damp or edge_damp;
 * border outside 0..size/2; max_records outside 0..2^28; null records with max_records > 0; hs at or above the
 * bound. After OCEAN_ERR_HIP (a launch failed part way) the maps hold an unfinished step and the accumulators
 * are zeroed again; reset the window before using it further.
 *
 *     dt, substeps   (s) the call advances dt in `substeps` substeps            defaults 1/60, 4
 *     gravity        (m/s^2)                                                     9.8
 *     rho_g          (N/m^3) the hulls'                                          9810
 *     damp           (1/s) on the velocity, everywhere                           0.05
 *     edge_damp      (1/s) added at the window's edge, falling to 0 over border  8
 *     border         (texels) width of the absorbing frame                       16 */
typedef struct ocean_wake_settings {
  float dt;
  int32_t substeps;
  float gravity;
  float rho_g;
  float damp;
  float edge_damp;
  int32_t border;
  int32_t reserved;  /* not read */
} ocean_wake_settings;
void ocean_default_wake_settings(ocean_wake_settings* out);
typedef struct ocean_wake ocean_wake;
int ocean_wake_create(ocean_wake** out, ocean_fft* fft, int size, float dx, float origin_x, float origin_z,
                      float smoothing);
/* Waits for the plan's stream, then frees the window. A null wake is accepted. */
int ocean_wake_destroy(ocean_wake* wake);
int ocean_wake_size(const ocean_wake* wake);   /* M; 0 for a null wake */
/* The taps T[a][b], a, b in 0..6, row-major, as the device uses them. Needs no device. */
int ocean_wake_kernel(const ocean_wake* wake, float out[49]);
double ocean_wake_max_substep(const ocean_wake* wake, float gravity);
int ocean_wake_origin(const ocean_wake* wake, float out[2]);   /* (ox, oz) of texel (0, 0) */
/* Device, size x size floats, the current h; null for a null wake. A step of an odd number of substeps makes
 * the other map current, so the pointer is valid until the next ocean_wake_step: ask again after it. The
 * caller may write it in stream order (an initial condition, a restored state). */
float* ocean_wake_height(ocean_wake* wake);
/* h = h_prev = 0: one memset on the plan's stream; ocean_wake_sample's dh/dt is 0 until the next step. */
int ocean_wake_reset(ocean_wake* wake);
/* off_i += di and off_j += dj, and both maps move: h'[i, j] = h[i + di, j + dj] where that lies inside, else
 * 0. |di|, |dj| <= 2^20; a shift of M or more in either direction clears the window, (0, 0) launches nothing.
 * It follows a body by whole texels, so the contents never resample. Two launches through the accumulators'
 * storage and a memset that leaves it zero. */
int ocean_wake_shift(ocean_wake* wake, int di, int dj);
int ocean_wake_step(ocean_wake* wake, const ocean_wake_settings* settings, const float* records,
                    const int64_t* count_device, int64_t max_records);
/* xz: device, n x 2 floats of base points (slots 0 and 2 of ocean_surface_query); out: device, n x 4 floats
 * (h, dh/dx, dh/dz, dh/dt). In unfused fp32:
 *     u = (x - ox) / dx;   v = (z - oz) / dx
 *     inside iff u >= 0 && u <= (float)(M-1), and the same for v; outside, or NaN, gives four zeros
 *     i0 = min((int)floorf(u), M-2), fx = u - (float)i0, and likewise j0, fz; hab = h[i0+a, j0+b]
 *     x0 = h00 + fx * (h10 - h00);   x1 = h01 + fx * (h11 - h01);   h = x0 + fz * (x1 - x0)
 *     gx = ((h10 - h00) + fz * ((h11 - h01) - (h10 - h00))) / dx
 *     gz = ((h01 - h00) + fx * ((h11 - h10) - (h01 - h00))) / dx
 *     dh/dt = the bilinear form of h over (h - h_prev) per tap, divided by the last call's hs; 0 before any
 *             step and after a reset
 * n in 0..2^31-1. One launch. OCEAN_ERR_INVALID for a null wake, n outside its range, null xz or out with n > 0. */
int ocean_wake_sample(ocean_wake* wake, const float* xz, int64_t n, float* out);
/* A window without a plan and without device storage, for checking the argument rules, the taps and the bound
 * where there is no device: ocean_wake_create's rules and taps; ocean_wake_kernel, _max_substep, _origin, _size
 * and _destroy work on it; every call that would launch is refused with OCEAN_ERR_INVALID after its other
 * checks. */
int ocean_debug_wake_create_host(ocean_wake** out, int size, float dx, float origin_x, float origin_z,
                                 float smoothing);

/* ---- Persistent foam: per-cascade accumulation, coverage counts, sampler ------------------------
 * The Jacobian map and slot 3 of the samplers say where the surface is folding now. Foam is a history:
 * whitecaps are born where the surface compresses, ride with the water and fade over seconds. The
 * reference declares that state (src/Generator.h:88-92: "we accumulate foam into a texture. This foam
 * decays over time exponentially") and never builds it: computeFoam writes the instantaneous determinant
 * and the fragment shader drops it. The maps are indexed by base point (a texel is the rest position of a
 * water particle), so foam kept per texel rides with its particle: no advection pass. Like the Jacobian,
 * foam is per cascade.
 *
 * Settings, per cascade; ocean_settings keeps its 64 bytes. The defaults (0.9, 8.0, 0.5, 0.5) are
 * starting points, not measurements: the counts below exist to tune them.
 *     bias   the Jacobian below which the surface feeds foam
 *     gain   (1/s) foam per unit of (bias - J) per second
 *     decay  (1/s) exponential decay rate
 *     level  the foam value from which a texel counts as covered */
typedef struct ocean_foam_settings {
  float bias;
  float gain;
  float decay;
  float level;
} ocean_foam_settings;
void ocean_default_foam_settings(ocean_foam_settings* out);
/* Mutable, like ocean_generator_settings: read by the next ocean_generator_advance_foam. Null, with
 * ocean_last_error set, for a null generator or a cascade out of range. */
ocean_foam_settings* ocean_generator_foam_settings(ocean_generator* gen, int cascade);
/* One step of every cascade's foam map. Contract, per cascade c and texel, with J the current Jacobian
 * texel and F the foam texel (R32F, N*N, row-major, 0 at first), in unfused fp32:
 *     a  = (float) exp(-(double)decay_c * (double)dt)      on the host, double libm exp, rounded once
 *     s  = max(bias_c - J, 0.0f) * gain_c
 *     t  = F * a + s * dt                                  three roundings: two products, one sum
 *     F' = min(t, 1.0f)
 *     breaking += (bias_c - J > 0);   covered += (F' >= level_c);   saturated += (t >= 1.0f)
 * dt == 0 leaves F bit for bit unchanged (a = 1 and s * 0 = 0): the reference app's `Q` freeze. Maps
 * holding NaN, and subnormal products, are unspecified.
 * Enqueued on the generator's stream after the row pass that wrote the Jacobian it reads (the ordering
 * of ocean_generator_build_bounds): two kernel launches, 12 B per point (J read, F read and written), no
 * host synchronisation, no float and no integer atomics. It does not rewrite the maps, so mips, rates
 * and bounds stay fresh. Foam is state, not a derived product: the next frame does not make it stale, and
 * re-seeding h0 or editing settings does not clear it.
 * The storage (4 B per point and cascade, the count table and 12 B per 2048 texels of partial counts) is
 * allocated and zeroed on the first ocean_generator_advance_foam or ocean_generator_reset_foam
 * (OCEAN_ERR_OOM when that fails) and freed by ocean_generator_destroy. Whole-grid generators only, every N
 * in 16 .. 16384 and every frame path.
 * OCEAN_ERR_INVALID, before any device call: a null generator; a slab generator; a generator that has
 * calculated no frame yet; dt negative or non-finite; a cascade (named in the message) whose bias or level
 * is non-finite or whose gain or decay is negative or non-finite. No reference counterpart. */
int ocean_generator_advance_foam(ocean_generator* gen, float dt);
/* Zeroes the foam maps and the counts, on the generator's stream. Allowed before any frame; allocates
 * the storage on first use. OCEAN_ERR_INVALID for a null or a slab generator. */
int ocean_generator_reset_foam(ocean_generator* gen);
/* R32F N*N, row-major, device memory, valid until the generator is destroyed; the cascades' maps are
 * consecutive. Null, with ocean_last_error set, for a null generator, a cascade out of range, and before
 * the first ocean_generator_advance_foam or ocean_generator_reset_foam. */
float* ocean_generator_foam_map(ocean_generator* gen, int cascade);
/* Host copy of (breaking, covered, saturated) of one cascade's last step; all zeros after a reset.
 * Synchronises the generator's stream. OCEAN_ERR_INVALID for a null generator or output, a cascade out of
 * range, and before the first ocean_generator_advance_foam or ocean_generator_reset_foam. */
int ocean_generator_foam_counts(ocean_generator* gen, int cascade, int64_t out[3]);
/* The table [cascade][3] in device memory, valid until the generator is destroyed (the step's partial
 * counts, uint32 [cascade][max(N*N / 2048, 1)][3], follow it). Null, with ocean_last_error set, for a null
 * generator and before the first ocean_generator_advance_foam or ocean_generator_reset_foam. */
const int64_t* ocean_generator_foam_counts_device(ocean_generator* gen);
/* ocean_surface_sample / ocean_surface_sample_plane with the foam in slot 7, which those calls leave 0;
 * the other seven floats are theirs bit for bit.
 *     foam = sum over the pairs c, in order, of tap_c(F_c) / (float)count
 * accumulated exactly as the fragment stage accumulates the Jacobian: at the displaced position, with
 * the same taps and weights. Argument rules, (generator, cascade) rules and stream as
 * ocean_surface_sample; the maps are sampled directly (no atlas). Every generator must have foam storage
 * (an ocean_generator_advance_foam or ocean_generator_reset_foam): otherwise OCEAN_ERR_INVALID, naming the
 * index of the generator in `gens`, before any device call. points == 0 launches nothing.
 * No reference counterpart. */
int ocean_surface_sample_foam(ocean_generator* const* gens, const int* cascades, int count, const float* xz,
                              int64_t points, float* out);
int ocean_surface_sample_plane_foam(ocean_generator* const* gens, const int* cascades, int count,
                                    const float camera[5], int res, float* out);

/* ---- Foam deposit: spray impacts splatted into the persistent foam --------------------------------
 * ocean_generator_advance_foam feeds the foam from the Jacobian alone. ocean_particles_step's impact list
 * (landed_out: the point and velocity of every particle that hit the water, with its count on the device)
 * says where spray comes down; ocean_foam_deposit adds foam there, without the host. The foam samplers and
 * the camera's foam stage then see it with no change to any of them.
 *
 * Settings, per (generator, cascade) pair of a call. The defaults (0.05, 0.01) are starting points, not
 * measurements.
 *     amount     foam one impact adds, spread over the four texels around it
 *     per_speed  (s/m) more foam per m/s of downward speed at the impact */
typedef struct ocean_foam_deposit_settings {
  float amount;
  float per_speed;
} ocean_foam_deposit_settings;
void ocean_default_foam_deposit_settings(ocean_foam_deposit_settings* out);
/* records: max_records x 8 floats in device memory, in the layout of landed_out; only slots 0, 2 and 5 are
 * read (px, pz, uy). The number of records is n = min(*count_device, max_records), read on the device
 * (a negative count is 0); a null count_device means n = max_records. For an impact list pass
 * ocean_particles_counts_device(pool) + 4. settings: host, one per pair.
 * Contract, in unfused fp32, per record r < n and per pair i in order, with L the pair's planeSize, F its
 * foam map and s = settings[i]. The taps (o_k, w_k), k = 0..3, are the texels and weights with which the
 * foam sampler reads F at the displaced position (px, pz): GL_LINEAR + GL_REPEAT at (px / L, pz / L). The
 * deposit is the transpose of the sampler: it takes a world position, not a base point.
 *     d   = s.amount + s.per_speed * max(-uy, 0.0f)        one product, one sum
 *     m_k = min(d * w_k, 1.0f)
 *     u_k = (uint64)(m_k * 16777216.0f)                    truncation; units of 2^-24, at most 2^24 per tap
 *     A[i][o_k] += u_k                                     an integer sum over all records and taps
 * and then for every texel t with A[i][t] > 0
 *     F[t] = min(F[t] + (float)min(A[i][t], 2^24) * 0x1p-24f, 1.0f)
 * Both conversions are exact and 2^28 records x 2^24 units cannot overflow 64 bits, so the result does not
 * depend on the order of the records and a call replays bit for bit. A pair with amount == 0 and
 * per_speed == 0 receives nothing and its map is not touched; texels without units keep their bits.
 * Non-finite positions or velocities are unspecified; their taps still stay inside the maps.
 * Counts: int64[50] in device memory owned by gens[0]:
 *     [0] n   [1] offered (*count_device, or max_records when it is null)
 *     [2 + 3i] taps with u_k > 0   [3 + 3i] texels touched   [4 + 3i] touched texels with F + add >= 1
 * per pair i; the three values are 0 for i >= count.
 * (generator, cascade) rules and stream as ocean_particles_step; every generator must have foam storage
 * (ocean_surface_sample_foam's rule and message, naming the index in `gens`); two pairs may not name the same
 * map. Three kernel launches: integer atomic adds into one uint64 accumulator per texel, an exchange that
 * makes one lane the owner of each touched texel (so the work scales with the records, not with N * N), and
 * the fold of the counts. No host synchronisation and no float atomics. The accumulators, 8 B per point and
 * cascade of every generator with a depositing pair (1 GiB at 8 x 4096^2), and gens[0]'s counts are
 * allocated and zeroed on the first call that needs them (OCEAN_ERR_OOM when that fails), are all zero
 * between calls and are freed by ocean_generator_destroy; no allocation after that. It does not rewrite the
 * generator's maps, so mips, rates and bounds stay fresh. max_records == 0 launches nothing and zeroes the
 * counts.
 * OCEAN_ERR_INVALID, before any device call: null gens / cascades / settings; count outside 1..16;
 * max_records negative or above 2^28, or null records with max_records > 0; an amount or per_speed that is
 * negative or non-finite. No reference counterpart. */
int ocean_foam_deposit(ocean_generator* const* gens, const int* cascades, int count,
                       const ocean_foam_deposit_settings* settings, const float* records,
                       const int64_t* count_device, int64_t max_records);
/* Host copy of the last call's counts with gen0 as gens[0]; synchronises the generator's stream.
 * OCEAN_ERR_INVALID for a null generator or output and before the first such call. */
int ocean_foam_deposit_counts(ocean_generator* gen0, int64_t out[50]);
/* The table in device memory, valid until the generator is destroyed. Null, with ocean_last_error set, for a
 * null generator and before the first call with gen0 as gens[0]. */
const int64_t* ocean_foam_deposit_counts_device(ocean_generator* gen0);
/* Measurement switch (default on): 0 issues one atomic per tap instead of folding runs of neighbouring
 * records on one texel within the wave first (the same words either way; tools/foam_deposit_bench.py times
 * both). Returns the previous value. */
int ocean_debug_foam_deposit_merge(int enable);

/* ---- Spray emitters: ordered compaction of breaking texels into records -------------------------
 * The Jacobian map says where the surface is folding now, the foam keeps its history, and
 * ocean_surface_velocity gives the position and velocity of the water particle under a base point. A
 * consumer that spawns something at breaking crests (spray, whitecap sprites, splash sounds, radar
 * sea-clutter scatterers) wants those joined: a list of emitters, each the point where the surface breaks
 * now with the velocity that throws the particle. ocean_spray_emit builds that list on the device: dense,
 * in a fixed order, thinned by a per-texel probability, with a count that stays on the device.
 *
 * Settings, per (generator, cascade) pair of a call. The defaults (0.9, 8.0, 0) are starting points, not
 * measurements.
 *     threshold  a texel can emit where threshold - J > 0
 *     rate       (1/s) emission probability per second per unit of (threshold - J); 0: the pair never emits
 *     seed       of the pair's random numbers */
typedef struct ocean_spray_settings {
  float threshold;
  float rate;
  uint32_t seed;
} ocean_spray_settings;
void ocean_default_spray_settings(ocean_spray_settings* out);
/* An emitter is its own object, like a hull set: it owns the scratch of the compaction (12 B per 2048
 * texels for 16 pairs of the plan's N, and the count table), which is allocated on the first
 * ocean_spray_emit (OCEAN_ERR_OOM when that fails). Calls run on the stream of `fft`.
 * OCEAN_ERR_INVALID for a null out or fft. */
typedef struct ocean_spray ocean_spray;
int ocean_spray_create(ocean_spray** out, ocean_fft* fft);
/* Waits for the plan's stream, then frees the emitter. */
int ocean_spray_destroy(ocean_spray* spray);
/* settings: host, one per pair. tiles: host, count x 2 int32 (tx, tz), or null for all zero: pair i's
 * texels stand for the copy of its periodic plane shifted by (tx, tz) plane sizes. out: device,
 * capacity x 8 floats.
 *
 * Contract, in unfused fp32. For each pair i in order, with J its Jacobian map, L its planeSize,
 * s = settings[i], and each texel (x, y) in row-major order:
 *     d = s.threshold - J[y*N + x]
 *     p = fminf((fmaxf(d, 0.0f) * s.rate) * dt, 1.0f)                  two products
 *     n = hash(hash(x, y) ^ s.seed, step)                             hash: the generator's counter hash,
 *     u = (float)((n >> 1) & 0x7FFFFFFF) / (float)0x7FFFFFFF           resources/spectrum.compute:109-115
 *     emits = d > 0 && (p >= 1.0f || u < p)
 * u can round to 1.0, hence the p >= 1 arm: a large finite rate emits every breaking texel. The emitting
 * texels form one list ordered by (pair, y*N + x) ascending; found is its length and
 * written = min(found, capacity). Record r < written is 8 floats:
 *     cell = L / (float)N
 *     bx = ((float)x + 0.5f) * cell + (float)tiles[i][0] * L          two products, one sum
 *     bz = ((float)y + 0.5f) * cell + (float)tiles[i][1] * L
 *     velocity != 0:  (px, py, pz, 0, ux, uy, uz, 0) = ocean_surface_velocity over all pairs at (bx, bz)
 *     velocity == 0:  (px, py, pz) = ocean_surface_sample's vertex stage over all pairs; ux = uy = uz = +0
 *     out[r] = (px, py, pz, d,  ux, uy, uz, bits of the uint32 (i << 28 | y*N + x))
 * So slots 0-2 and 4-6 are ocean_surface_velocity's (velocity == 0: slots 0-2 ocean_surface_sample's) bits
 * at the texel's centre, slot 3 is positive, and slot 7 names the pair and the texel (pairs <= 16 and
 * N*N <= 2^28). Records from `written` on are not touched. A pair with rate == 0 emits nothing and its map
 * is not read; it still takes part in every record's position and velocity.
 * Counts: int64[18] in device memory: [0] written, [1] found, [2 + i] pair i's share of found (0 for
 * i >= count). capacity == 0 with out == null is a counting-only call.
 * Maps holding NaN, and (d * rate) * dt that is not finite, are unspecified. Subsequent calls overwrite
 * the counts; the scratch serves one call at a time, in stream order.
 *
 * (generator, cascade) rules and stream as ocean_hulls_loads: whole-grid generators, all of the plan's N,
 * 1..16 pairs, gens[0] on the emitter's plan. At most four kernel launches (count per 2048-texel item,
 * scan of the items, scatter of (d, id), dense fill of the records; two for a counting-only call), the
 * kernel boundaries being the only ordering: no host synchronisation, no float and no integer atomics, no
 * allocation after the first call. The same call on the same maps gives the same bytes on every run and
 * under every CU budget. The count pass reads 4 B per texel of the emitting pairs, the scatter at most
 * 4 B per texel; a record costs 32 B written and its taps.
 * OCEAN_ERR_INVALID, before any device call, naming the index in `gens` where one applies: a null
 * emitter; null gens / cascades or count outside 1..16; null settings; a negative capacity; a null out
 * with capacity > 0; dt negative or non-finite; a non-finite threshold; a rate that is negative or
 * non-finite; the (generator, cascade) rules; a generator that has calculated no frame yet; with
 * velocity != 0, rates that were never calculated or are stale (the rule of ocean_surface_velocity).
 * No reference counterpart. */
int ocean_spray_emit(ocean_spray* spray, ocean_generator* const* gens, const int* cascades, int count,
                     const ocean_spray_settings* settings, const int32_t* tiles, float dt, uint32_t step,
                     int velocity, int64_t capacity, float* out);
/* Host copy of the last call's counts; synchronises the plan's stream. OCEAN_ERR_INVALID for a null
 * emitter or output and before the first ocean_spray_emit. */
int ocean_spray_counts(ocean_spray* spray, int64_t out[18]);
/* The counts in device memory, valid until the emitter is destroyed. Null, with ocean_last_error set, for
 * a null emitter and before the first ocean_spray_emit. */
const int64_t* ocean_spray_counts_device(ocean_spray* spray);

/* ---- Spray particles: a persistent pool, stepped, landed on the water, compacted in order --------
 * ocean_spray_emit says where spray is born and with what velocity; a pool carries it further. One call per
 * frame, ocean_particles_step, moves every live particle under gravity and linear drag toward a wind, finds
 * the water under it with ocean_surface_query's fixed point, compacts the survivors in their order into the
 * next list and the particles that hit the water, in their order, into an impact list, and appends the
 * records of an ocean_spray_emit call, whose count it reads on the device.
 *
 * Settings, one struct per call. The defaults (9.8, 0.5, no wind, 4, 1, 10, 4, 1e-3) are starting points,
 * not measurements.
 *     gravity     (m/s^2) downward
 *     drag        (1/s) linear, toward the wind
 *     wind        (m/s)
 *     lifetime    (s) a particle whose age reaches it expires; +inf: never
 *     gain        launch velocity = gain * the emitter record's velocity
 *     lift        (m/s) upward, per unit of the emitter record's d = threshold - J (slot 3)
 *     iterations  of the surface query under a particle, 0..64
 *     tolerance   (m) of that query */
typedef struct ocean_particle_settings {
  float gravity;
  float drag;
  float wind[3];
  float lifetime;
  float gain;
  float lift;
  int32_t iterations;
  float tolerance;
} ocean_particle_settings;
void ocean_default_particle_settings(ocean_particle_settings* out);
/* A pool is its own object, like an emitter. It is created with everything it ever needs: two lists of
 * capacity x 8 floats (the current and the next one), the scratch of the compaction (88 B per 256
 * particles) and the count table; OCEAN_ERR_OOM when an allocation fails. A fresh pool is empty and its
 * counts are all zero. Calls run on the stream of `fft`. OCEAN_ERR_INVALID for a null out or fft and for a
 * capacity outside 1..2^28. */
typedef struct ocean_particles ocean_particles;
int ocean_particles_create(ocean_particles** out, ocean_fft* fft, int64_t capacity);
/* Waits for the plan's stream, then frees the pool. A null pool is accepted. */
int ocean_particles_destroy(ocean_particles* pool);
/* emit_records: device, the `out` of an ocean_spray_emit call, or null; emit_counts_device: that emitter's
 * ocean_spray_counts_device. landed_out: device, landed_capacity x 8 floats.
 *
 * Contract, in unfused fp32. A particle is 8 floats (px, py, pz, age, ux, uy, uz, id). With s = *settings,
 * `alive` the length of the list, and each particle r < alive in list order:
 *     ax = s.drag * (s.wind[0] - ux)
 *     ay = s.drag * (s.wind[1] - uy) - s.gravity
 *     az = s.drag * (s.wind[2] - uz)
 *     ux' = ux + ax * dt   (uy', uz' likewise)                         one product, one sum each
 *     px' = px + ux' * dt  (py', pz' likewise)                         semi-implicit Euler
 *     age' = age + dt
 *     w = slot 1 of ocean_surface_query over the call's pairs at q = (px', pz') with s.iterations and
 *         s.tolerance: a cold start at q, the height at the last V(p), converged or not
 *     landed   = !(py' > w)                                            a NaN lands
 *     expired  = !landed && !(age' < s.lifetime)
 *     survives = neither
 * Survivors keep their order: survivor k becomes record k of the next list,
 *     (px', py', pz', age', ux', uy', uz', id).
 * Landed particles keep theirs: landed k < min(landed, landed_capacity) is written to landed_out[k] as
 *     (px', w, pz', age', ux', uy', uz', id),
 * the point and velocity of impact; records of landed_out from there on are not touched.
 * landed_capacity == 0 with landed_out == null only counts.
 * Append: with emit_records non-null and E = emit_counts_device[0] (the emitter's `written`, read on the
 * device), appended = min(E, capacity - survivors), and emitter record e < appended,
 * (px, py, pz, d, ux, uy, uz, id), becomes particle survivors + e:
 *     (px, py, pz, +0, s.gain * ux, s.gain * uy + s.lift * d, s.gain * uz, id)    two products, one sum
 * with the id's bits unchanged. Appended particles are not moved in this call. A null emit_records appends
 * nothing, and emit_counts_device is then not read.
 * Counts: int64[8] in device memory: [0] alive after the call (survivors + appended), [1] alive before it,
 * [2] survivors, [3] landed found, [4] landed written, [5] expired, [6] appended, [7] dropped
 * (E - appended). Always [1] == [2] + [3] + [5]. dt == 0 still classifies and compacts.
 * Positions that are not finite give an unspecified w (their taps stay inside the maps).
 *
 * (generator, cascade) rules and stream as ocean_spray_emit: whole-grid generators, all of the plan's N,
 * 1..16 pairs, gens[0] on the pool's plan, every generator with a frame calculated. Three kernel launches
 * (move and classify per 256-particle item; scan of the items with the count table; scatter with the
 * append), the kernel boundaries being the only ordering: no host synchronisation, no atomics, no
 * allocation. The same call on the same list and maps gives the same bytes on every run and under every CU
 * budget. A particle costs 32 B read and 32 B written in the first launch beside the query's taps, and, if
 * it survives or lands, 32 B read and 32 B written in the third.
 * OCEAN_ERR_INVALID, before any device call, naming the index in `gens` where one applies: a null pool; null
 * gens / cascades or count outside 1..16; null settings; dt negative or non-finite; a non-finite gravity,
 * wind, gain or lift; a drag that is negative or non-finite; a lifetime that is not > 0 (+inf accepted);
 * iterations outside 0..64; a tolerance that is negative or non-finite; a negative landed_capacity; a null
 * landed_out with landed_capacity > 0; a non-null emit_records with a null emit_counts_device; the
 * (generator, cascade) rules; a generator that has calculated no frame yet.
 * No reference counterpart. */
int ocean_particles_step(ocean_particles* pool, ocean_generator* const* gens, const int* cascades, int count,
                         const ocean_particle_settings* settings, float dt, const float* emit_records,
                         const int64_t* emit_counts_device, int64_t landed_capacity, float* landed_out);
/* Replaces the list with `count` caller records (device, count x 8 floats), in stream order: restoring a
 * saved state. The counts become (count, 0, 0, ..). OCEAN_ERR_INVALID for a null pool, a count outside
 * 0..capacity, or null records with count > 0. */
int ocean_particles_load(ocean_particles* pool, const float* device_records, int64_t count);
/* Empties the list: ocean_particles_load with count 0. */
int ocean_particles_clear(ocean_particles* pool);
/* The current list in device memory, counts[0] records: valid until the next ocean_particles_step,
 * ocean_particles_load or ocean_particles_destroy on the pool (a step makes the other list current). Null,
 * with ocean_last_error set, for a null pool. */
const float* ocean_particles_records(ocean_particles* pool);
/* Host copy of the counts; synchronises the plan's stream. OCEAN_ERR_INVALID for a null pool or output. */
int ocean_particles_counts(ocean_particles* pool, int64_t out[8]);
/* The counts in device memory, valid until the pool is destroyed. Null, with ocean_last_error set, for a
 * null pool. */
const int64_t* ocean_particles_counts_device(ocean_particles* pool);

#ifdef __cplusplus
}
#endif

#endif /* OCEANFFT_H */
