/*
 * rdc_amd.h — C ABI of the MI355X-native rdc allreduce path (librdc_amd.so).
 *
 * The reference ships NO C ABI: its Python package calls `_LIB.Rdc*` symbols
 * that exist nowhere in src/ (SURVEY.md §0 finding 3).  The entry points below
 * are exactly the ones those callers bind, with the signatures the call sites
 * imply, plus device-resident extensions for the MI355X path.
 * Plain pointers and sizes only; no torch types.
 *
 * Conventions
 *   - every function returns 0 on success and a non-zero code on failure
 *     (RdcGetLastError() then describes it), except the getters
 *     RdcGetRank/RdcGetWorldSize/RdcIsDistributed/RdcCommRank/RdcCommSize;
 *     the reference aborts via CHECK_F instead — the C++ header include/rdc.h
 *     restores that behaviour on top of these codes.
 *   - dtype: mpi::DataType (include/core/mpi.h:19-30) = rdc/core.py:160-169:
 *       0 int8, 1 uint8, 2 int32, 3 uint32, 4 int64, 5 uint64, 6 float32,
 *       7 float64, 8 long long, 9 unsigned long long
 *     MI355X additions: 10 float16 (IEEE binary16), 11 bfloat16, and the
 *     (value, index) pairs of MAXLOC / MINLOC, the value first, 8 bytes:
 *       12 F32_I32 { float value; int32_t index; }
 *       13 I32_I32 { int32_t value; int32_t index; }
 *     or 16 bytes (a 64-bit index numbers every element the library can move;
 *     float64 scores keep their bits):
 *       16 F64_I64 { double value; int64_t index; }
 *       17 I64_I64 { int64_t value; int64_t index; }
 *     A buffer of pairs, host or device, must be aligned to the pair's size: 8
 *     bytes for 12 / 13, 16 bytes for 16 / 17.  The C struct alone guarantees 4
 *     / 8 (declare it alignas(8) / alignas(16), as rdc::ValueIndex<V> is): a
 *     less aligned pair buffer is refused as "not aligned to its element
 *     size" before anything is launched; for 16 / 17 RdcAllreduce refuses it
 *     at a world size of 1 too.  Codes 14 and 15 are unassigned and refused as
 *     "bad dtype 14" / "bad dtype 15".  Not covered: the padded
 *     { double, int32 } of MPI_DOUBLE_INT, whose padding bytes have no defined
 *     bits, and a { float, int64 } pair.
 *   - op: mpi::OpType (include/core/mpi.h:12-17) = rdc/core.py:16-20:
 *       0 MAX, 1 MIN, 2 SUM, 3 BITOR (integer dtypes only)
 *     MI355X additions (MPI_MAXLOC / MPI_MINLOC): 4 MAXLOC, 5 MINLOC.
 *       MAXLOC: dst = src when dst.value < src.value ||
 *                             (dst.value == src.value && src.index < dst.index)
 *       MINLOC: the same with > in the first comparison.
 *     So: a NaN in dst.value stays and a NaN in src.value is ignored, as for
 *     MAX / MIN; -0.0f == +0.0f is a tie in value and the lower index wins; on
 *     a full tie (equal value, equal index) dst stays whole, value bits
 *     included, so a +0 / -0 pair with equal indexes depends on the operand
 *     order, as NaN does for MAX.  On 16 / 17 the comparisons are IEEE double
 *     and signed 64-bit, on all 64 bits of value and index.  MAXLOC / MINLOC
 *     are valid with dtypes 12, 13, 16 and 17 only, and those dtypes with
 *     MAXLOC / MINLOC only: every other combination is refused before anything
 *     is launched, the message naming both.  RdcFill has no pattern for the
 *     pair dtypes and refuses them (upload the inputs); RdcCommAutotune times
 *     no pair candidates and refuses them too.
 *     MI355X additions (MPI_PROD / MPI_BAND / MPI_BXOR), dst = OP(dst, src):
 *       8 PROD   dst * src   every arithmetic dtype 0-11
 *       9 BITAND dst & src   integer dtypes only, as BITOR
 *      10 BITXOR dst ^ src   integer dtypes only
 *     Codes 6 and 7 are unassigned and refused as "bad op 6" / "bad op 7"
 *     (both have long served callers as the example of an unknown operator);
 *     11 and above likewise.
 *     PROD on integers wraps modulo 2^bits (computed on the unsigned type, as
 *     SUM).  On float32, float64 and float16 it is one IEEE multiply,
 *     round-to-nearest-even, subnormals kept.  On bfloat16 it is the float32
 *     product of the two widened values (exact), rounded to bfloat16 once
 *     (RNE): the correctly rounded product.  NaN payloads are not pinned.  The
 *     fold orders are SUM's (ring order per chunk, tree order at or below
 *     rdc_reduce_ring_mincount, rank order for scans), and they decide a
 *     floating product's bits exactly as they decide a sum's.  BITAND / BITXOR
 *     with a float dtype and any of the three with a pair dtype are refused
 *     before anything is launched.
 *   - results are bit-identical to the reference's CPU ring allreduce
 *     (src/comm/communicator_collective.cc:115-203) on the same inputs.
 */
#ifndef RDC_AMD_H_
#define RDC_AMD_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ */
/* Reference-bound entry points (the names rdc/core.py & rdc/comm.py call) */
/* ------------------------------------------------------------------ */

/* rdc::Init (include/rdc.h:58-61, include/core/rdc-inl.h:21-23;
 * rdc/core.py:29-49 calls RdcInit(len(args), arr)).  argv entries of the form
 * key=val override environment variables (communicator_manager.cc:87-104).
 * Keys: RDC_RANK, RDC_WORLD_SIZE|rdc_world_size, RDC_TRACKER_URI,
 * RDC_TRACKER_PORT, rdc_reduce_ring_mincount, RDC_DEVICE, RDC_SCRATCH_BYTES,
 * RDC_ALGO (mesh|mesh_pull|ring|oneshot), RDC_NBLOCKS, RDC_TILE_BYTES, RDC_TIMEOUT, RDC_ONESHOT_BYTES,
 * RDC_FUSE_BYTES, RDC_FUSE_BYTES_DIRECT, RDC_COALESCE_FUSED, RDC_HOST_ZC_BYTES,
 * RDC_BCAST_SPLIT_BYTES, RDC_P2P_SLOT_BYTES.
 * Falls back to torchrun's RANK/WORLD_SIZE/LOCAL_RANK/MASTER_ADDR/MASTER_PORT
 * (tracker port = MASTER_PORT+1).  Does not touch the GPU. */
int RdcInit(int argc, char** argv);
/* rdc::Finalize (include/rdc.h:75; rdc/core.py:52-57) */
int RdcFinalize(void);
/* rdc::GetRank / GetWorldSize / IsDistributed (include/rdc.h:76-80;
 * rdc/core.py:66-87) */
int RdcGetRank(void);
int RdcGetWorldSize(void);
int RdcIsDistributed(void);
/* rdc::TrackerPrint (include/api.h:9; rdc/core.py:90-103) */
int RdcTrackerPrint(const char* msg);
/* rdc/core.py:106-118 */
int RdcGetProcessorName(char* buf, unsigned long* out_len, unsigned long max_len);
/* rdc::Barrier (include/api.h:14) */
int RdcBarrier(void);

/* rdc::Allreduce<OP,DType> (include/api.h:62-64, include/core/rdc-inl.h:125-135)
 * on the "main" communicator; rdc/core.py:204-216 calls
 * RdcAllreduce(ptr, size, dtype_enum, int(op), prepare_fun|NULL, NULL).
 * sendrecv may be host or device memory (detected); synchronous, in place.
 * prepare_fun(prepare_arg), when given, runs before the reduction. */
int RdcAllreduce(void* sendrecv, size_t count, int dtype, int op, void (*prepare_fun)(void*),
                 void* prepare_arg);
/* rdc::Broadcast(void*, size, root) (include/api.h:23-24, rdc-inl.h:71-75;
 * rdc/core.py:143-154).  Host or device memory; synchronous. */
int RdcBroadcast(void* sendrecv, unsigned long size, int root);

/* The same two calls on a named communicator (rdc::Allreduce<OP,DType>(buf,
 * count, comm_name), include/api.h:62-64; rdc::Broadcast(..., comm_name),
 * include/api.h:23-26).  Host or device memory; synchronous. */
int RdcAllreduceOn(void* comm, void* sendrecv, size_t count, int dtype, int op);
int RdcBroadcastOn(void* comm, void* sendrecv, size_t size, int root);

/* rdc::Allgather (include/api.h:47-52, include/core/rdc-inl.h:106-122;
 * TryAllgatherRing, communicator_collective.cc:79-114): bufs[c] holds
 * sizes[c] bytes; on entry bufs[rank] holds this rank's data, on return every
 * bufs[c] holds rank c's data.  All host or all device memory; synchronous.
 * RdcAllgather uses the "main" communicator. */
int RdcAllgather(void** bufs, const size_t* sizes);
int RdcAllgatherOn(void* comm, void** bufs, const size_t* sizes);

/* In-place reduce-scatter (Communicator::TryReduceScatterRing,
 * src/comm/communicator_collective.cc:115-182; include/comm/communicator_base.h:
 * 217-233: "after the function, node k get k-th segment of the reduction
 * result"; the reference reaches it only as the first half of its ring
 * allreduce).  Chunk c = utils::Split(0, count, n)[c] (RdcPlanSplit), the
 * allreduce's chunk map.  On return chunk `rank` of sendrecv holds the
 * reduction of that chunk over all ranks, bit-identical to chunk `rank` of
 * what RdcAllreduce returns on the same inputs by the ring order,
 * x[r] (+) (x[r+1] (+) ... (+) x[r-1]).  The ring order applies at EVERY size:
 * TryReduceScatterRing has no tree branch, so rdc_reduce_ring_mincount does
 * not apply.  Every byte of sendrecv outside chunk `rank` is left exactly as
 * the caller passed it (the reference leaves ring partials there).  count = 0
 * or world size 1 succeed without touching the GPU; with count < n some chunks
 * are empty and their ranks still take part.  Host or device memory
 * (detected); synchronous.  A host buffer goes up whole, and only chunk `rank`
 * is copied back.  RdcReduceScatter uses the "main" communicator. */
int RdcReduceScatter(void* sendrecv, size_t count, int dtype, int op);
int RdcReduceScatterOn(void* comm, void* sendrecv, size_t count, int dtype, int op);

/* In-place reduction to one rank (MPI_Reduce, ncclReduce; named ReduceTo
 * because RdcReduce is the local element-wise reduce).  On rank `root` all
 * count elements of sendrecv receive the reduction over all ranks,
 * bit-identical to what RdcAllreduce leaves there by the ring order: element e
 * of chunk c = utils::Split(0, count, n)[c] is x[c] (+) (x[c+1] (+) ... (+)
 * x[c-1]).  The ring order applies at EVERY size: rdc_reduce_ring_mincount is
 * not consulted.  On every other rank sendrecv is only read: every byte stays
 * exactly as the caller passed it.  `root` must be the same on every rank (the
 * caller's contract, as for RdcBroadcast).  The (dtype, op) pairs are the
 * allreduce's.  Refused with a message in RdcGetLastError before anything is
 * launched: a root outside [0, n), an unsupported (dtype, op), a buffer not
 * aligned to its element size, a null buffer with count > 0.  count = 0 or
 * world size 1 succeed without touching the GPU.  Host or device memory
 * (detected); synchronous.  A host buffer goes up whole on every rank and the
 * whole result is copied back on the root only: a non-root host buffer is
 * never written.  RdcReduceTo uses the "main" communicator. */
int RdcReduceTo(void* sendrecv, size_t count, int dtype, int op, int root);
int RdcReduceToOn(void* comm, void* sendrecv, size_t count, int dtype, int op, int root);

/* Sum of float16 (dtype 10) / bfloat16 (dtype 11) buffers with a float32
 * accumulator (MI355X addition).  The ordinary Sum rounds to 16 bits at every
 * hop (the reference's rule: n - 1 roundings); here the owner of a chunk adds
 * the n raw contributions in binary32 and rounds ONCE.  THE RULE, for element
 * e of chunk c = utils::Split(0, count, n)[c], x[q] rank q's value:
 *     s = f32(x[c-1]);  for j = 2..n:  s = f32(x[c-j]) + s     (indices mod n)
 *     result = round_to_T(s)
 * f32() is exact; every add is an IEEE binary32 add, round to nearest even,
 * subnormals kept; round_to_T is one round-to-nearest-even conversion
 * (overflow gives inf; a NaN stays a NaN, its payload is not pinned).  The
 * sequence x[c-1], x[c-2], ..., x[c] is the ring order every schedule folds
 * in, so each element has one defined bit pattern that tiling and piece cuts
 * cannot change.  rdc_reduce_ring_mincount is not consulted: there is no tree
 * branch.  At n = 2 the result is bit-identical to the ordinary Sum (one
 * binary32 add of two 16-bit values, rounded once, is their correctly rounded
 * 16-bit sum).  For n > 2 the result is the rounding of the float32 fold,
 * which is not always the correctly rounded exact sum.
 * Three collectives, each with its sibling's chunk map, result placement and
 * untouched bytes: RdcAllreduceAcc32 (every rank receives all count elements),
 * RdcReduceScatterAcc32 (chunk `rank` receives its elements, every byte
 * outside it stays exactly as passed), RdcReduceToAcc32 (rank `root` receives
 * all count elements, every other rank's buffer is only read).  Refused with
 * a message in RdcGetLastError before anything is launched: a dtype other
 * than 10 / 11 ("rdc: float32-accumulated Sum needs float16 or bfloat16, got
 * dtype N"), a root outside [0, n), a buffer not aligned to its element size,
 * a null buffer with count > 0.  count = 0 or world size 1 succeed without
 * touching the GPU.  Host or device memory (detected); synchronous.  A host
 * buffer goes up whole on every rank and comes back where the siblings copy
 * back: whole (allreduce), chunk `rank` only (reduce-scatter), whole on the
 * root only (reduce-to: a non-root host buffer is never written).  The calls
 * without a handle use the "main" communicator. */
int RdcAllreduceAcc32(void* sendrecv, size_t count, int dtype);
int RdcAllreduceAcc32On(void* comm, void* sendrecv, size_t count, int dtype);
int RdcReduceScatterAcc32(void* sendrecv, size_t count, int dtype);
int RdcReduceScatterAcc32On(void* comm, void* sendrecv, size_t count, int dtype);
int RdcReduceToAcc32(void* sendrecv, size_t count, int dtype, int root);
int RdcReduceToAcc32On(void* comm, void* sendrecv, size_t count, int dtype, int root);

/* Avg: the mean across ranks of float32 (dtype 6), float64 (7), float16 (10)
 * or bfloat16 (11) buffers (MI355X addition; ReduceOp.AVG / ncclAvg elsewhere).
 * Every other reduction here leaves a sum, and a caller who wants the mean
 * divides in a second pass: one more launch, one more trip of the buffer
 * through memory, a second rounding of 16-bit results, and a float16 sum that
 * overflowed before the division could save it (four ranks of 40000.0: Sum
 * and RdcAllreduceAcc32 give inf, the mean is 40000.0).  On the mesh the owner
 * of a chunk holds all n raw contributions and is the only place a result is
 * produced, so the division happens there, before the single store.  THE
 * RULE, for element e of chunk c = utils::Split(0, count, n)[c], x[q] rank q's
 * value, indices mod n:
 *   float32 / float64 (T):
 *     s = x[c-1];  for j = 2..n:  s = x[c-j] + s      in T: the ordinary Sum's
 *     result = s / T(n)                               ring-order bits, then one
 *                                                     IEEE division
 *   float16 / bfloat16 (T):
 *     s = f32(x[c-1]);  for j = 2..n:  s = f32(x[c-j]) + s   (RdcAllreduceAcc32's fold)
 *     q = s / float(n)                                       in binary32
 *     result = round_to_T(q)                                 one rounding, overflow -> inf
 * Every add and the division are IEEE operations, round to nearest even,
 * subnormals kept.  It is a DIVISION by n, not a multiplication by a rounded
 * 1 / n: the two differ in 20 - 55 % of random values at n = 3, 5, 6, 7, 12
 * (at a power-of-two n they are the same bits).  A 16-bit Avg always
 * accumulates in float32; there is no per-hop 16-bit Avg.  The ring order
 * holds at every size: rdc_reduce_ring_mincount is not consulted.  inf / n =
 * inf, inf - inf gives a NaN; NaN payloads are not pinned.
 * Three collectives, each with its sibling's chunk map, result placement and
 * untouched bytes: RdcAllreduceAvg (every rank receives all count elements),
 * RdcReduceScatterAvg (chunk `rank` receives its elements, every byte outside
 * it stays exactly as passed), RdcReduceToAvg (rank `root` receives all count
 * elements, every other rank's buffer is only read).  Refused with a message
 * in RdcGetLastError before anything is launched: any other dtype — integers
 * and the pair dtypes — ("rdc: Avg takes float32, float64, float16 or
 * bfloat16, got dtype N"), a root outside [0, n), a buffer not aligned to its
 * element size, a null buffer with count > 0.  count = 0 or world size 1
 * succeed without touching the GPU and leave the buffer unchanged (no
 * division by 1 is stored).  Host or device memory (detected); synchronous;
 * a host buffer is staged as for RdcAllreduceAcc32.  The calls without a
 * handle use the "main" communicator. */
int RdcAllreduceAvg(void* sendrecv, size_t count, int dtype);
int RdcAllreduceAvgOn(void* comm, void* sendrecv, size_t count, int dtype);
int RdcReduceScatterAvg(void* sendrecv, size_t count, int dtype);
int RdcReduceScatterAvgOn(void* comm, void* sendrecv, size_t count, int dtype);
int RdcReduceToAvg(void* sendrecv, size_t count, int dtype, int root);
int RdcReduceToAvgOn(void* comm, void* sendrecv, size_t count, int dtype, int root);

/* Prefix reduction across ranks, in place (MPI_Scan; exclusive = 1: MPI_Exscan;
 * MI355X addition: the reference has no scan).  With x[q] rank q's input, y[0]
 * = x[0] and y[q] = OP::Reduce(dst = y[q-1], src = x[q]): a left fold in rank
 * order, element by element, so tiling and piece cuts cannot change a bit.
 * Inclusive (exclusive = 0): rank r ends with y[r].  Exclusive (exclusive = 1):
 * rank r > 0 ends with y[r-1].  On rank 0 sendrecv is only read in both modes:
 * every byte stays exactly as passed (MPI leaves rank 0's exscan result
 * undefined; here it is defined).  The running prefix is always the dst
 * operand of op::Reducer: for Max / Min a NaN in the prefix sticks and a NaN in
 * x[q] is ignored; signed sums wrap; fp16 / bf16 round per hop.  For a
 * floating-point Sum y[n-1] does NOT have the bits RdcAllreduce leaves (its
 * ring order starts each chunk at another rank; this fold always starts at
 * rank 0).  rdc_reduce_ring_mincount is not consulted: the reference has no
 * scan and no tree branch applies.  The (dtype, op) pairs are the allreduce's.
 * Refused with a message in RdcGetLastError before anything is launched: an
 * unsupported (dtype, op), a buffer not aligned to its element size, a null
 * buffer with count > 0, `exclusive` outside {0, 1}.  count = 0 or world size 1
 * succeed without touching the GPU and consume no launch number.  Host or
 * device memory (detected); synchronous.  A host buffer goes up whole on every
 * rank and the whole result is copied back on every rank but 0: rank 0's host
 * buffer is never written.  RdcScan uses the "main" communicator. */
int RdcScan(void* sendrecv, size_t count, int dtype, int op, int exclusive);
int RdcScanOn(void* comm, void* sendrecv, size_t count, int dtype, int op, int exclusive);

/* All-to-all, out of place (MI355X addition: the reference has no personalised
 * exchange; its custom-reducer allreduce builds one out of ISend / IRecv).
 * On rank r, bytes [send_off[p], send_off[p] + send_len[p]) of `send` land at
 * [recv_off[r], recv_off[r] + recv_len[r]) of rank p's `recv`; arrays of n
 * entries, offsets and lengths in bytes.  Contract, as in MPI: send_len[p] on
 * rank r equals recv_len[r] on rank p — a rank cannot check it.  A
 * violation never hangs or faults and never leaves the slot or the receive
 * segment, but only one kind of it is reported: a receiver that expects more
 * tiles than were sent ends in the bounded-wait error (RDC_TIMEOUT).  Where
 * the sender's length is the longer one (or the tile counts happen to be
 * equal) every expected tile arrives, and the receiver lands recv_len[r] bytes
 * of undefined content — a truncated segment — with no error.  Rank r's own segment is a local copy (send_len[r] must equal
 * recv_len[r]).  Zero-length segments are legal, a whole zero row or column
 * and an all-zero call included: an alltoallv is still collective and is
 * exactly ONE device launch.  After the call every byte of `recv` outside the
 * n receive segments is as the caller left it and `send` is unchanged.
 * Refused before anything is launched: a null buffer with bytes to move, send
 * and receive ranges that overlap (each side's extent is the hull of its
 * segments), receive segments that overlap each other, own-segment lengths
 * that differ, and a segment longer than one launch carries
 * (RdcPlanAlltoallCap: about 255 MiB at 8 ranks with the default scratch).
 * The refusal is local: the peers of a rank that refused report the
 * bounded-wait error, as for any call not made collectively; callers slice
 * larger exchanges.  RdcAlltoall is the equal split, segment p at
 * p * bytes_per_peer on both sides, any size (every rank cuts the same
 * ceil(bytes_per_peer / cap) launches; none for 0 bytes).
 * Host or device memory (detected; host buffers are staged through HBM like
 * RdcAllgather's); synchronous.  World size 1: the own-segment copy only (no
 * GPU needed for host memory).  RdcAlltoall[v] use the "main" communicator. */
int RdcAlltoall(const void* send, void* recv, size_t bytes_per_peer);
int RdcAlltoallOn(void* comm, const void* send, void* recv, size_t bytes_per_peer);
int RdcAlltoallv(const void* send, const size_t* send_off, const size_t* send_len, void* recv,
                 const size_t* recv_off, const size_t* recv_len);
int RdcAlltoallvOn(void* comm, const void* send, const size_t* send_off, const size_t* send_len, void* recv,
                   const size_t* recv_off, const size_t* recv_len);

/* Coalesced (bucketed) allreduce: the result of one RdcAllreduce per buffer,
 * in order, bit-identical, but the buffers move in fused launches (BASELINE
 * cfg5 / test/mallreduce.cc's back-to-back shape).  A list takes the schedule
 * and launch shape one buffer of its total size would get (the automatic rule,
 * or what RdcCommAutotune chose for that size class); the mesh and the ring
 * read and write the buffers in place through a cached unit table (groups of
 * up to RDC_FUSE_BYTES_DIRECT, default 16 GiB); one-shot lists are packed
 * chunk-major into an HBM staging image in groups of RDC_FUSE_BYTES (default
 * 256 MiB).  Buckets whose addresses are 16-B aligned take the vector paths;
 * a bucket that is only element-aligned folds element by element (correct,
 * slower): RdcCommGetParam(comm, "coalesced_misaligned") counts them in the
 * last coalesced call.
 * bufs[b] holds counts[b] elements of `dtype`; all host or all device memory;
 * synchronous.  RdcAllreduceCoalesced uses the "main" communicator. */
int RdcAllreduceCoalesced(void** bufs, const size_t* counts, int nbuf, int dtype, int op);
int RdcAllreduceCoalescedOn(void* comm, void** bufs, const size_t* counts, int nbuf, int dtype, int op);

/* rdc::NewCommunicator / GetCommunicator (include/rdc.h:62-71;
 * rdc/comm.py:90-93,106-109 call RdcNewCommunicator(byref(handle), name)).
 * NewCommunicator is collective over all ranks.  Named communicators over the
 * same ranks share one scratch channel (one pool of uncached HBM per rank):
 * every rank must then issue the collectives of ALL those communicators in
 * the same order (the SPMD order rdc programs follow; the reference's
 * Allreduce is not thread-safe either, communicator.h:87).  Ranks that
 * interleave two communicators differently — e.g. from two threads — need
 * RDC_SHARE_SCRATCH=0 (a channel per communicator, as the reference's
 * independent TCP meshes behave). */
int RdcNewCommunicator(void** out, const char* name);
int RdcGetCommunicator(void** out, const char* name);
/* rdc::CreateGroup / ICommunicator::CreateGroup (include/api.h:124-125,
 * include/comm/communicator.h:133-134; declared, never defined in the
 * reference): a communicator over `ranks` (ranks of `parent`, NULL = "main";
 * group rank i = ranks[i]) named `name` ("" = "group<k>").  Collective over
 * every rank of the parent, all passing the same list; *out = NULL on ranks
 * not in it.  Members rendezvous through node-local shared memory and get
 * their own scratch; destroy with RdcCommDestroy (collective over members). */
int RdcCreateGroup(void** out, void* parent, const int* ranks, int nranks, const char* name);

/* Point-to-point (ICommunicator::ISend/IRecv, include/comm/communicator.h:
 * 56-80; rdc/comm.py:46-80 binds RdcISend / RdcIRecv / RdcWorkCompletion*).
 * Buffers are rdc Buffer handles (rdc/buffer.py:34-38: RdcNewBuffer(byref(h),
 * addr, size, pinned)) over host OR device memory; `pinned` page-locks a host
 * range (hipHostRegister) for the buffer's lifetime (whole pages only: a
 * page-aligned address and size).  A host allreduce (RdcAllreduce /
 * RdcCommAllreduce on a host pointer) whose buffer lies inside such a range
 * DMAs straight from and into it, with no copy through staging memory.  Data moves GPU to GPU
 * over xGMI through the receiver's IPC-mapped slots; messages on one (src,
 * dst) pair are matched in order and must have equal sizes on both sides.
 * A request that makes no progress for RDC_TIMEOUT seconds ends in error.
 * Completion handles are freed with RdcDelWorkCompletion (safe while
 * pending).  RdcIRecv returns the handle (NULL on failure), as comm.py:73
 * expects; every other function returns a status code. */
int RdcNewBuffer(void** out, void* addr, size_t size, int pinned);
int RdcDelBuffer(void* buf);
int RdcISend(void** wc, void* comm, void* buf, int dest);
void* RdcIRecv(void* comm, void* buf, int src);
/* 0 = finished, 1 = error (RdcWorkCompletionError describes it) */
int RdcWorkCompletionWait(void* wc);
/* WorkStatus (include/core/work_request.h:23-30): 2 pending, 8 finished, 64 error */
int RdcWorkCompletionStatus(void* wc);
const char* RdcWorkCompletionError(void* wc);
int RdcDelWorkCompletion(void* wc);
/* blocking rdc::Send / rdc::Recv on "main" (include/api.h:10-11) */
int RdcSend(void* buf, size_t size, int dest);
int RdcRecv(void* buf, size_t size, int src);
/* raw-pointer forms on `comm`; for device memory the copies start after the
 * work already queued on `stream` (NULL = default stream) */
int RdcCommISend(void** wc, void* comm, const void* buf, size_t bytes, int dest, void* stream);
int RdcCommIRecv(void** wc, void* comm, void* buf, size_t bytes, int src, void* stream);

/* ------------------------------------------------------------------ */
/* MI355X device-resident extensions                                    */
/* ------------------------------------------------------------------ */

/* In-place allreduce of device memory on `comm`, enqueued on `stream`
 * (hipStream_t; NULL = default stream).  Asynchronous: errors raised inside
 * the kernels (a peer that never joins) surface at RdcCommCheck. */
int RdcCommAllreduce(void* comm, void* dev_buf, size_t count, int dtype, int op, void* stream);
/* algo: 0 auto, 1 ring (the reference schedule), 2 mesh (all links, pushed by remote stores),
 * 6 direct (registered buffers, one process per rank: every rank's buffer is mapped into every
 * peer through HIP IPC once per allocation — a host rendezvous over shared memory agrees on the
 * buffers each call — and owner r folds chunk r straight out of the n buffers and writes the
 * result back into all of them: no scratch, one read and one write of each buffer; falls back
 * to the automatic rule on every rank when any buffer cannot be mapped, the addresses differ mod
 * 16, the stream is being captured or the ranks share one process; RDC_DIRECT_BYTES=<n> takes it
 * automatically from n bytes),
 * 5 pull-mode mesh (the same exchange by remote loads: ranks stage their chunks in their own
 * scratch, owners load and fold, peers load the results; RdcCommAutotune times it against
 * the push mesh), 3 one-shot (small buffers:
 * every rank pushes the whole buffer to every peer, one hand-off); auto = one-shot when
 * the one-shot while bytes <= 8 MiB and its extra egress over the mesh,
 * (n-1)(n-2)/n x bytes, is <= 4 MiB (n = 2: 8 MiB, n = 8: 0.76 MiB; with
 * RDC_ONESHOT_BYTES set: while (n-1) x bytes <= it), else the ring at n = 2
 * and the mesh from n = 3.  All bit-identical.
 * Whatever the algo, a buffer of at most rdc_reduce_ring_mincount bytes (default 1) takes
 * the reference's TREE order (TryAllreduce, src/comm/communicator_collective.cc:6-13: the
 * fold of TryReduceTree to rank 0, every rank receiving the root's bits) as one one-shot
 * style hand-off; algo 4 forces that tree order for any size. */
int RdcCommAllreduceEx(void* comm, void* dev_buf, size_t count, int dtype, int op, int algo, void* stream);
/* Device-resident in-place reduce-scatter (see RdcReduceScatter for the
 * result; TryReduceScatterRing, communicator_collective.cc:115-182),
 * stream-ordered; errors raised inside the kernels surface at RdcCommCheck.
 * algo: 0 auto; 2 mesh, pushed (the scratch schedule: every rank pushes the
 * other chunks to their owners, owner r folds chunk r into its own buffer;
 * works in single-process groups and can be captured in a hipGraph; a launch
 * ends only after every peer's launch ended, so the scratch slots need no gate
 * in whatever launch follows); 6 direct (registered buffers, one process per
 * rank: owner r folds chunk r straight out of the n buffers and stores it into
 * its own only).  Auto takes direct exactly where RdcCommAllreduceEx's auto
 * does (same channel check, the RdcPlanDirectAuto threshold — measured for the
 * allreduce, provisional here —, never while capturing), else the mesh; a
 * direct call that cannot run (a refused mapping, buffers that differ mod 16,
 * a released channel) falls back to the mesh on every rank and is counted in
 * "direct_fallback".  algo 1, 3, 4 and 5 are invalid arguments: the ring would
 * clobber the other chunks, the one-shot and the tree make no sense for a
 * scatter, and the pull mesh is dominated by direct wherever direct can run.
 * RdcCommLastLaunch then reports algo 2 or 6 and 0 gather blocks. */
int RdcCommReduceScatter(void* comm, void* dev_buf, size_t count, int dtype, int op, int algo, void* stream);
/* device-resident coalesced allreduce (see RdcAllreduceCoalesced), stream-ordered.
 * The per-group unit table is cached by (buffers, counts): after a first
 * (warm-up) call with the same buckets, launches need no host->device copy
 * and can be captured in a hipGraph.  algo 6 (or an Autotune'd direct
 * schedule for the list's total size) runs the whole list as ONE direct
 * launch between the ranks' buffers (every buffer's allocation mapped into
 * the peers, <= 4096 buffers in <= 64 allocations per call; else the
 * scratch schedules). */
int RdcCommAllreduceCoalesced(void* comm, void* const* dev_bufs, const size_t* counts, int nbuf, int dtype, int op,
                              int algo, void* stream);
int RdcCommBroadcast(void* comm, void* dev_buf, size_t bytes, int root, void* stream);
/* device-resident allgather of per-rank buffers (see RdcAllgather), stream-ordered */
int RdcCommAllgather(void* comm, void** dev_bufs, const size_t* sizes, void* stream);
/* Device-resident in-place reduction to `root` (see RdcReduceTo for the result
 * and the refusals), stream-ordered; errors raised inside the kernel surface
 * at RdcCommCheck.  One schedule, on the scratch path: the mesh allreduce with
 * its second half narrowed to one destination — every rank pushes the other
 * chunks to their owners, owner r folds chunk r in its ring order, the root
 * into its own buffer and every other owner into the root's scratch only,
 * which the root copies into its buffer.  Works in single-process groups and
 * can be captured in a hipGraph.  A launch ends only after every peer's launch
 * ended, so the scratch slots need no gate in whatever launch follows.
 * RdcCommTune / RDC_NBLOCKS / RDC_TILE_BYTES apply as for a mesh allreduce of
 * the same bytes.  RdcCommLastLaunch reports algo 2, and gather blocks on the
 * root only. */
int RdcCommReduceTo(void* comm, void* dev_buf, size_t count, int dtype, int op, int root, void* stream);
/* Device-resident float32-accumulated Sum of float16 / bfloat16 (see
 * RdcAllreduceAcc32 for the rule, the results and the refusals),
 * stream-ordered; errors raised inside the kernels surface at RdcCommCheck.
 * One schedule each, the pushed mesh (algo 2) at every size and every n, n = 2
 * included: RdcCommAllreduceEx's mesh, RdcCommReduceScatter's and
 * RdcCommReduceTo's launches with the owner's fold widened — same bytes, same
 * hand-offs, same plans (RdcPlanAllreduce algo 2 / RdcPlanReduceScatter /
 * RdcPlanReduceTo), same launch kinds.  No one-shot, ring, tree, pull or
 * direct schedule and no resident host service, so a small call pays the
 * mesh's two hand-offs.  Works in single-process groups and can be captured in
 * a hipGraph.  RdcCommTune / RDC_NBLOCKS / RDC_TILE_BYTES apply as for a mesh
 * Sum of the same bytes; RdcCommLastLaunch reports what the mesh sibling
 * reports. */
int RdcCommAllreduceAcc32(void* comm, void* dev_buf, size_t count, int dtype, void* stream);
int RdcCommReduceScatterAcc32(void* comm, void* dev_buf, size_t count, int dtype, void* stream);
int RdcCommReduceToAcc32(void* comm, void* dev_buf, size_t count, int dtype, int root, void* stream);
/* Device-resident Avg (see RdcAllreduceAvg for the rule, the results and the
 * refusals), stream-ordered; errors raised inside the kernels surface at
 * RdcCommCheck.  One schedule each, the pushed mesh (algo 2) at every size and
 * every n, n = 2 included: the mesh siblings' launches with the owner's fold
 * followed by the division — same bytes, same hand-offs, same plans, same
 * launch kinds; the divisor is the communicator's size.  No one-shot, ring,
 * tree, pull or direct schedule and no resident host service.  Works in
 * single-process groups and can be captured in a hipGraph.  RdcCommTune /
 * RDC_NBLOCKS / RDC_TILE_BYTES apply as for a mesh Sum of the same bytes;
 * RdcCommLastLaunch reports what the mesh sibling reports. */
int RdcCommAllreduceAvg(void* comm, void* dev_buf, size_t count, int dtype, void* stream);
int RdcCommReduceScatterAvg(void* comm, void* dev_buf, size_t count, int dtype, void* stream);
int RdcCommReduceToAvg(void* comm, void* dev_buf, size_t count, int dtype, int root, void* stream);
/* Device-resident in-place scan / exscan (see RdcScan for the result and the
 * refusals), stream-ordered; errors raised inside the kernel surface at
 * RdcCommCheck.  One schedule, on the scratch path (k_scan): the ring's reduce
 * step without the wrap-around, pipelined tile by tile down the rank order —
 * rank 0 copies a tile into rank 1's scratch, rank r folds what it received
 * with its own tile, stores its result and, in the same pass, the prefix into
 * rank r+1's scratch.  Buffers beyond one scratch slot run as several launches.
 * Works in single-process groups and can be captured in a hipGraph.  A launch
 * ends only after every peer's launch ended, so the scratch slots need no gate
 * in whatever launch follows.  RdcCommTune / RDC_NBLOCKS / RDC_TILE_BYTES apply
 * as for a ring allreduce of the same bytes, except that a configured tile has
 * no 16 KiB floor.  RdcCommLastLaunch reports {grid, grid, 0, 0, tile bytes,
 * 103}. */
int RdcCommScan(void* comm, void* dev_buf, size_t count, int dtype, int op, int exclusive, void* stream);
/* Device-resident all-to-all (see RdcAlltoall / RdcAlltoallv for the result,
 * the contract and the refusals), stream-ordered; the scratch path (k_alltoall:
 * every rank pushes segment p into peer p's allgather slot `rank` and lands its
 * own slots; works in single-process groups).  The image of a segment starts at
 * its slot's base, so the 16-B vector path runs on a side whose segment address
 * is 16-B aligned and the narrower word paths otherwise.  Capture in a
 * hipGraph is untested.  RdcCommAlltoallv is exactly one launch per call (an all-zero call
 * included); RdcCommLastLaunch then reports {grid, push blocks, 0, land blocks,
 * tile bytes, 102}.  The offset / length arrays are read before the call
 * returns. */
int RdcCommAlltoall(void* comm, const void* send, void* recv, size_t bytes_per_peer, void* stream);
int RdcCommAlltoallv(void* comm, const void* send, const size_t* send_off, const size_t* send_len, void* recv,
                     const size_t* recv_off, const size_t* recv_len, void* stream);
/* synchronise `stream` and report any device-side collective failure */
int RdcCommCheck(void* comm, void* stream);
/* A communicator's parameter: "rdc_reduce_ring_mincount", "RDC_SCRATCH_BYTES",
 * "RDC_TILE_BYTES", "RDC_NBLOCKS", "RDC_ONESHOT_BYTES", "slot_bytes",
 * "ranks_per_gpu" (most ranks of it sharing one physical GPU), "coalesced_misaligned"
 * (buckets of the last coalesced call not 16-B aligned), "shares_scratch"
 * (1 when another communicator uses the same scratch channel: every named
 * communicator over the same ranks shares one, RDC_SHARE_SCRATCH=0 disables),
 * "host_registered_calls" (host allreduces of this process that DMA'd in place
 * from a pinned RdcNewBuffer range), "RDC_DIRECT_BYTES" (RDC_DIRECT_MIN_AUTO =
 * the default rule), "direct_check" (the channel's direct self-check, run at
 * creation: 0 not run, 1 passed, 2 failed), "flags_kind" / "scratch_kind" (3 =
 * HSA-uncached, MTYPE UC; 0 = hipDeviceMallocUncached, MTYPE CC on gfx950),
 * and the direct schedule's counters "direct_calls", "direct_rendezvous_ns",
 * "direct_export_ns", "direct_retired", "direct_closed", "direct_refused",
 * "direct_close_wait_ns", "direct_maps", "direct_exports", "direct_fallback"
 * (calls that fell back, alike on every rank), "direct_unusable" (of them, the
 * calls whose buffer lists could not run direct), "direct_map_failed" and
 * "direct_fail_reason" (this rank's peer-mapping failures and the last one's
 * code: 1 table full, 2 refused earlier, 3 open failed, 4 a mapping already
 * held, 5 lands partly over unmapped ranges, 6 the mapping did not show
 * the exporter's canary: another buffer object), "direct_canary" (new peer
 * mappings checked by their canary), "direct_export_failed" /
 * "direct_export_error" (exports of this rank's allocations HIP refused and
 * the last hipError_t), "direct_import" (1: peers mapped from dma-bufs at
 * chosen addresses, RDC_DIRECT_IMPORT=vmem; 0: HIP IPC) and "direct_pending"
 * (dma-bufs received and not mapped). */
int RdcCommGetParam(void* comm, const char* key, uint64_t* value);
int RdcCommRank(void* comm);
int RdcCommSize(void* comm);
int RdcCommDevice(void* comm);
/* 0 uncached, 1 fine-grained, 2 coarse-grained scratch */
int RdcCommAllocKind(void* comm);

/* xGMI link probe (diagnostics, bench.py at N > 1): push `bytes` per target
 * from this rank's scratch into peers' scratch `reps` times on `stream`, all
 * targets at once, with the copy kernel the collectives use for remote
 * stores.  mode 0: rank+1 only (one link, one direction); mode 1: every peer
 * (all n-1 links out of this GPU); modes 2 / 3: the same links read instead
 * (pull from rank+1 / from every peer into local scratch).  *ms_out = average ms per round;
 * *bytes_out (may be NULL) = bytes per target actually pushed (clamped to
 * the scratch slot).  Call it
 * between collectives with every rank idle (e.g. after a barrier): it
 * overwrites scratch, which every collective rewrites before reading. */
int RdcCommProbe(void* comm, int mode, size_t bytes, int reps, void* stream, double* ms_out, size_t* bytes_out);

/* Re-tune one communicator between collectives (every rank of it must pass
 * the same values; the plan is made per call on each host): mesh role split
 * in sixteenths of the grid (RDC_MESH_SPLIT; mesh_s16 + mesh_r16 <= 15, the
 * gather role gets the rest), grid size (RDC_NBLOCKS; 0 = auto) and tile
 * bytes (RDC_TILE_BYTES; 0 = auto, else a multiple of 256).  Results stay
 * bit-identical (the fold order is per element).  No reference counterpart:
 * the reference's schedule has no such knobs; bench.py sweeps them at N>1. */
int RdcCommTune(void* comm, int mesh_s16, int mesh_r16, int max_blocks, size_t tile_bytes);

/* Debug mode (RDC_POISON_SCRATCH; every rank of `comm` should pass the same
 * value, though ranks that differ stay correct): with on != 0 every consumer
 * of a hand-off overwrites the scratch range it finished reading with 0xFF
 * bytes before the signal that lets the producer reuse it, so a read of a
 * range before its producer's next publish lands NaN / all-ones words instead
 * of a plausible older value.  Results are unchanged; each launch stores its
 * consumed scratch bytes once more.  No reference counterpart. */
int RdcCommSetPoison(void* comm, int on);

/* The direct schedule (algo 6) maps each peer's buffer into this process once
 * per allocation and keeps the mapping while the communicator lives; a
 * mapping keeps the peer's allocation alive after the peer frees it, and an
 * allocation at an address this rank exported before for another allocation
 * is not exported again (those calls take the scratch schedules).  This
 * closes all of this rank's mappings (after waiting for the device) and turns
 * the direct schedule off for the communicator, releasing the peers' freed
 * allocations.  Call it on every rank.  No reference counterpart. */
int RdcCommDirectRelease(void* comm);

/* Autotune (collective: every rank of `comm`, same arguments, no collective in
 * flight; blocks the host): time the ring, the mesh pushed and pulled (RDC_ALGO_MESH_PULL),
 * (where it fits half a slot) the one-shot schedule and (ranks in processes of
 * their own) the direct schedule, then the launch shapes of the fastest, for
 * `bytes` of `dtype` on this node — mesh: role split, then grid, then
 * tiles per reduce block; ring: grid, then tiles per block (a granularity, so
 * the chosen tiles scale with later buffers' sizes) — `reps` Max allreduces of synthetic data each on a scratch
 * buffer, in 3 rounds per candidate taken round-robin over each stage; agree
 * on the per-round times with a MAX allreduce over `comm` (identical on every
 * rank, so every rank keeps the same winner); a candidate's time is the median
 * of its rounds, and each stage keeps its first candidate (stage 0: the
 * automatic rule's schedule; later: the previous winner) unless another is
 * faster by more than 3 %; keep the chosen schedule and shape for allreduces of that size class ([2^k,
 * 2^(k+1)) bytes; other sizes keep the automatic rule and the configured
 * shape, RdcCommTune clears every autotuned one, and nothing is tuned while
 * RDC_ALGO forces a schedule; with RDC_TUNE_FILE set, rank 0 appends the
 * winner there and later communicators of the same rank and CU count start
 * from it).  cand (room for max_cand; 24 suffices)
 * receives every timed candidate with its slowest-rank ms; *ncand their count,
 * *best the chosen index (-1 and nothing changed for sizes that take the
 * tree order, rdc_reduce_ring_mincount).  Results stay bit-identical whatever wins.  No
 * reference counterpart (the reference's schedule has no launch shape). */
typedef struct {
    int algo;                           /* RDC_ALGO_RING (1), RDC_ALGO_MESH (2), RDC_ALGO_ONESHOT (3),
                                           RDC_ALGO_MESH_PULL (5) */
    int mesh_s16, mesh_r16, max_blocks; /* max_blocks 0 = automatic grid */
    int tiles_per_block;                /* 0 = default (mesh 2 per reduce block, ring 1) */
    double ms;                          /* per allreduce: median over rounds of the slowest rank's time */
    double ms_min, ms_max;              /* spread of that time over the rounds */
} RdcTuneCand;
int RdcCommAutotune(void* comm, size_t bytes, int dtype, int reps, void* stream, RdcTuneCand* cand, int max_cand,
                    int* ncand, int* best);

/* Diagnostics (bench.py at N > 1): the next allreduce on `comm` (mesh or
 * ring schedule) records, per block, {start, end} wall_clock64 ticks
 * (100 MHz) into dev_words (device memory, >= 2 x grid uint64 words; a launch
 * with a larger grid is not traced).  RdcCommLastLaunch: {grid, nb_scatter,
 * nb_reduce, nb_gather, tile_bytes, algo} of the last allreduce launch
 * (mesh roles: blocks [0, s) scatter, [s, s+r) reduce, the rest gather). */
int RdcCommTraceNext(void* comm, void* dev_words, size_t nwords);
int RdcCommLastLaunch(void* comm, uint64_t* out6);

/* Diagnostics: the device launch counter of comm's scratch channel — the
 * counter half of every 64-bit hand-off sequence word (seq = counter << 8 |
 * communicator tag; 56-bit counters, compared modulo 2^56, so flag slots never
 * written or idle for any number of launches never read as "reached").
 * RdcCommSetLaunchCounter is collective: every rank of the channel sets the
 * same value with no collective in flight (tests start it past 2^32). */
int RdcCommLaunchCounter(void* comm, uint64_t* value);
int RdcCommSetLaunchCounter(void* comm, uint64_t value);

/* Single process driving n ranks (devices[i] = HIP device of rank i; devices
 * may repeat).  comms[i] receives rank i's handle.  scratch_bytes 0 = default. */
int RdcCommInitAll(void** comms, int n, const int* devices, size_t scratch_bytes);
/* Destroy a communicator (collective for communicators made by
 * RdcNewCommunicator; local for RdcCommInitAll groups). */
int RdcCommDestroy(void* comm);

/* op::Reducer<OP,DType>(src, dst, count) (include/core/mpi.h:113-120) on
 * device memory: dst[i] = OP::Reduce(dst[i], src[i]).  Stream-ordered. */
int RdcReduce(void* dst, const void* src, size_t count, int dtype, int op, void* stream);
/* Synchronous copy between any two of host / device memory (the C++ header's
 * custom-reducer path stages device buffers with it). */
int RdcMemcpy(void* dst, const void* src, size_t bytes);
/* Synthetic inputs: u = splitmix64(seed ^ (rank<<40) ^ i) mapped per dtype
 * (identical to the CPU oracle's generator).  Stream-ordered. */
int RdcFill(void* dev_buf, size_t count, int dtype, uint64_t seed, int rank, void* stream);

/* Host-side planning, no GPU needed (what the launches of a collective will
 * be; used by the CPU tests).  RdcPlanLayout: out = {slot_bytes,
 * region_bytes, max_tiles, flag_bytes} of a communicator of n ranks.
 * RdcPlanAllreduce: one record of RDC_PLAN_WORDS uint64 per launch:
 *   [tile_bytes, nb_scatter, nb_reduce, nb_gather,
 *    off[16], len[16], mis[16], tiles[16]]   (per chunk c < n)
 * *out_pieces = number of launches (records written: min(that, max_pieces)). */
#define RDC_PLAN_WORDS 68
/* Grid of a collective launch whose blocks wait on other ranks' blocks: the
 * requested grid `want` clamped so that every rank's blocks stay resident at
 * once, min(want, blocks_per_cu x cus / ranks_per_gpu) (at least 1).
 * Communicators apply it to every ring / mesh / one-shot / tree / broadcast /
 * allgather launch, including grids forced by RDC_NBLOCKS or RdcCommTune;
 * blocks_per_cu is the kernel's occupancy, ranks_per_gpu the most ranks of
 * the communicator on one physical GPU, cus the fewest CUs of any rank's GPU.
 * Returns the grid (not a status). */
int RdcPlanResidentGrid(int want, int blocks_per_cu, int cus, int ranks_per_gpu);
/* The clamp communicators apply (round 4): a dispatch sends workgroup i to
 * XCD i % xcds, so the grid is min(want, xcds x floor((blocks_per_cu x
 * cus / xcds - blocks_per_cu x reserve_cus) / ranks_per_gpu)) — every XCD
 * holds every rank's share even when the reserve_cus CUs kept for resident
 * service blocks all sit on one XCD (xcds = 1 when it does not divide cus).
 * With xcds = 1 and reserve_cus = 0 it is RdcPlanResidentGrid.  Communicators
 * pass hipDeviceAttributeNumberOfXccs (the most of any rank) and reserve one
 * CU per rank on the GPU. */
int RdcPlanResidentGridXcd(int want, int blocks_per_cu, int cus, int ranks_per_gpu, int xcds, int reserve_cus);
/* The tree allreduce's fold for n ranks (rdc_reduce_ring_mincount path): the
 * post-order program acc[dst[i]] = OP(acc[dst[i]], acc[src[i]]), i < n-1,
 * over the n ranks' inputs (acc[q] = rank q's value); the result is acc[0].
 * dst/src hold >= 16 ints.  Returns n-1, or -1 on bad arguments. */
int RdcPlanTree(int n, int* dst, int* src);
int RdcPlanLayout(int n, size_t scratch_bytes, uint64_t* out4);
/* The host-buffer pipeline's contiguous pieces for `bytes` (RDC_HOST_PIECE_BYTES,
 * RDC_HOST_PIECE_RAMP): bounds[0..*out_n) = {0, ..., bytes}, piece k = [bounds[k],
 * bounds[k+1]) (one piece up to 16 MiB).  Writes at most max_bounds entries. */
int RdcPlanHostPieces(size_t bytes, uint64_t* bounds, int max_bounds, int* out_n);
/* The ranges of one host-path piece [lo, hi) (byte offsets of a buffer of
 * `count` elements of `dtype`) over n ranks: off[q], len[q] (relative to lo)
 * owned by rank q and folded in the ring order of Split chunk fold[q].
 * balanced 0: the piece's bytes of chunk q go to rank q (fold[q] = q);
 * balanced 1: each chunk's bytes are cut over the ranks in proportion to
 * their length (RDC_HOST_BALANCE; the default with one rank per GPU). */
int RdcPlanHostPieceRanges(int n, size_t count, int dtype, uint64_t lo, uint64_t hi, int balanced, uint64_t* off,
                           uint64_t* len, int* fold);
/* The automatic schedule for an allreduce of `bytes` over n ranks: returns
 * RDC_ALGO_ONESHOT (3), RDC_ALGO_RING (1, n = 2 beyond the one-shot) or
 * RDC_ALGO_MESH (2) (negative on bad arguments).
 * oneshot_bytes = RDC_ONESHOT_BYTES (0 = the default size / rank-aware rule). */
int RdcPlanAutoAlgo(int n, size_t bytes, size_t scratch_bytes, size_t oneshot_bytes);
/* Whether an untuned automatic allreduce of `bytes` over n processes takes the
 * registered-buffer schedule (RDC_ALGO_DIRECT) when every rank's buffer can be
 * mapped and the channel's direct self-check passed: 1 / 0 (negative on bad
 * arguments).  direct_min = RDC_DIRECT_BYTES: RDC_DIRECT_MIN_AUTO (the
 * default) = beyond the one-shot sizes and from 16 MiB (32 MiB at n = 2); 0 = never; N = from N
 * bytes.  Replaces nothing in the reference (its one schedule is the ring);
 * the drop-in rdc::Allreduce / rdc.allreduce calls get it without tuning. */
#define RDC_DIRECT_MIN_AUTO (~(uint64_t)0)
int RdcPlanDirectAuto(int n, size_t bytes, size_t scratch_bytes, size_t oneshot_bytes, uint64_t direct_min);
/* HBM byte model of one allreduce of `count` elements over n ranks with
 * schedule `algo` (1 ring, 2 mesh, 3 one-shot, 4 tree, 5 pull-mode mesh, 6 direct): the
 * bytes the kernels load and store, counted per access as their loops issue
 * them, a remote store or load counted at the rank that issues it.  out5 = {read bytes, write bytes
 * (both the most of any rank), read bytes, write bytes (both summed over the
 * ranks), link egress bytes (the most of any rank)}.  bench.py's N > 1
 * roofline divides this by the measured time. */
int RdcPlanHbmBytes(int n, size_t count, int dtype, int algo, uint64_t* out5);
int RdcPlanAllreduce(int n, size_t count, int dtype, size_t scratch_bytes, int algo, size_t tile_bytes,
                     int max_blocks, uint64_t* out, int max_pieces, int* out_pieces);

/* utils::Split(0, count, n)[rank] (include/utils/utils.h:59-70) in 64-bit
 * arithmetic: the element range [*begin, *end) of chunk `rank`, the chunk a
 * reduce-scatter leaves on that rank and the allreduce's owner map. */
int RdcPlanSplit(size_t count, int n, int rank, uint64_t* begin, uint64_t* end);
/* The launches of a mesh reduce-scatter (RdcCommReduceScatter, algo 2), in
 * RdcPlanAllreduce's records: the offsets, lengths, mis and tiles of
 * RdcPlanAllreduce(algo 2) for the same arguments, nb_gather = 0, and the grid
 * split between scatter and reduce 1 : 2 (the default role split's s16 : r16). */
int RdcPlanReduceScatter(int n, size_t count, int dtype, size_t scratch_bytes, size_t tile_bytes, int max_blocks,
                         uint64_t* out, int max_pieces, int* out_pieces);
/* RdcPlanHbmBytes' model of one reduce-scatter, algo 2 (mesh: the scatter
 * loads the other chunks and stores them remotely, the fold loads n x chunk r
 * and stores it once) or 6 (direct: n x chunk r loaded, n-1 of them over the
 * link, chunk r stored once).  out5 as RdcPlanHbmBytes; egress = the bytes of
 * this rank's buffer that go to peers (pushed by it, or loaded by them). */
int RdcPlanReduceScatterBytes(int n, size_t count, int dtype, int algo, uint64_t* out5);

/* The launches of a rooted reduce (RdcCommReduceTo) on rank `rank`, in
 * RdcPlanAllreduce's records.  The offsets, lengths, mis, tiles and tile bytes
 * are RdcPlanAllreduce(algo 2)'s for the same arguments and depend on neither
 * rank nor root (both ends of every hand-off cut alike); the root gets the
 * mesh's scatter / reduce / gather split, every other rank RdcPlanReduceScatter's
 * (nb_gather = 0).  Refused: a rank or root outside [0, n), an unsupported
 * (dtype, op). */
int RdcPlanReduceTo(int n, int rank, int root, size_t count, int dtype, int op, size_t scratch_bytes,
                    size_t tile_bytes, int max_blocks, uint64_t* out, int max_pieces, int* out_pieces);
/* RdcPlanHbmBytes' model of one rooted reduce on rank `rank`: every rank loads
 * the other chunks and stores them remotely, and loads n x its own chunk; a
 * non-root rank stores the folded chunk remotely (both stores are egress); the
 * root stores it locally, loads its AG slots and stores the gathered chunks.
 * out5 as RdcPlanHbmBytes (for one rank max = sum); rank < 0: the maxima and
 * sums over all n ranks. */
int RdcPlanReduceToBytes(int n, int rank, int root, size_t count, int dtype, uint64_t* out5);

/* The launches of a scan / exscan (RdcCommScan) in RdcPlanAllreduce's records:
 * every piece uses off[0] / len[0] / tiles[0] (mis 0: its image starts at the
 * slot's base) and word 1 is its grid, min(tiles, max_blocks).  The pieces tile
 * the buffer in order; a piece has at most min(RdcPlanAlltoallCap, flag-row
 * length x tile) bytes.  Tile bytes: tile_bytes if not 0 (a multiple of 256),
 * else the piece's bytes / max_blocks rounded up to 256, within [64 KiB,
 * 1 MiB].  Nothing depends on `rank` (both ends of every hand-off cut alike);
 * it is only checked.  Refused: a rank outside [0, n), an unsupported (dtype,
 * op), tile_bytes not a multiple of 256. */
int RdcPlanScan(int n, int rank, size_t count, int dtype, int op, size_t scratch_bytes, size_t tile_bytes,
                int max_blocks, uint64_t* out, int max_pieces, int* out_pieces);
/* RdcPlanHbmBytes' model of one scan / exscan of S = count elements on rank
 * `rank`: rank 0 loads S and stores S remotely (egress); 0 < r < n-1 loads 2 S
 * and stores 2 S, one of them remotely; rank n-1 loads 2 S and stores S.  out5
 * as RdcPlanHbmBytes (for one rank max = sum); rank < 0: the maxima and sums
 * over all n ranks. */
int RdcPlanScanBytes(int n, int rank, size_t count, int dtype, uint64_t* out5);

/* The one launch of an all-to-all as rank `rank` plans it from its row
 * (send_len[n]) and column (recv_len[n]) of the size matrix.  out (36 words):
 * tile bytes, push blocks, land blocks, 0, then out_tiles[16] (tiles of the
 * segment for rank p; 0 for p = rank) and in_tiles[16] (tiles of the segment
 * from rank c; [rank]: the own segment's).  Tile bytes depend only on values
 * equal on every rank (tile_bytes, else 64 KiB; with equal_len != 0 — the
 * equal split's bytes per peer of this launch — one push item per push block
 * within [64 KiB, 1 MiB]), and a pair's tiles on the one length both ends
 * know, so sender and receiver cut alike. */
int RdcPlanAlltoall(int n, int rank, const uint64_t* send_len, const uint64_t* recv_len, size_t scratch_bytes,
                    size_t tile_bytes, int max_blocks, uint64_t equal_len, uint64_t* out36);
/* the largest segment one all-to-all launch carries: the allgather's per-piece
 * capacity, round_down(slot_bytes - 256, 256) of RdcPlanLayout(n, scratch_bytes) */
int RdcPlanAlltoallCap(int n, size_t scratch_bytes, uint64_t* cap);
/* RdcPlanHbmBytes' model of one all-to-all on rank `rank`: reads = the send
 * buffer + its own slots, writes = the peers' slots + the receive buffer,
 * egress = the bytes pushed to peers (out5 as RdcPlanHbmBytes; max = sum) */
int RdcPlanAlltoallBytes(int n, int rank, const uint64_t* send_len, const uint64_t* recv_len, uint64_t* out5);

/* RdcPlanCoalesced: the staging image of one fusion group.  chunk_out (33
 * words): packed chunk offsets off[16], lengths len[16], total bytes.  units_out:
 * 4 words per copy unit {buffer index, byte offset in the buffer, byte offset
 * in the image, bytes}.  RdcPlanFuseGroups: group boundaries (group g =
 * buffers [bounds[g], bounds[g+1])); fuse_bytes 0 = default. */
int RdcPlanCoalesced(int n, const size_t* counts, int nbuf, int dtype, uint64_t* chunk_out, uint64_t* units_out,
                     int max_units, int* out_units);
/* RdcPlanDirectItems: owner `rank`'s items of a coalesced direct launch
 * (algo 6 over a list): Split chunk `rank` of every buffer in pieces of at
 * most `tile` bytes, 3 words each {buffer, byte offset, bytes}. */
int RdcPlanDirectItems(int n, int rank, const size_t* counts, int nbuf, int dtype, uint64_t tile, uint64_t* out,
                       int max_items, int* out_items);
int RdcPlanFuseGroups(const size_t* counts, int nbuf, int dtype, size_t fuse_bytes, int* bounds_out, int max_bounds,
                      int* out_n);

/* Set a parameter (same keys as RdcInit argv). */
int RdcSetParam(const char* name, const char* value);
/* Description of the last failure on this thread ("" if none). */
const char* RdcGetLastError(void);
const char* RdcVersion(void);

#ifdef __cplusplus
}
#endif
#endif /* RDC_AMD_H_ */
