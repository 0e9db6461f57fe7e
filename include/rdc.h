/*!
 * rdc.h — the reference's C++ interface (include/rdc.h, include/api.h,
 * include/core/rdc-inl.h, include/core/mpi.h of akkaze/rdc) over the
 * MI355X device path in librdc_amd.so.
 *
 * Drop-in for the allreduce/broadcast surface: same namespaces, names,
 * template parameters and argument meaning.  Differences, all deliberate:
 *   - the collectives work on host OR device (hipMalloc'd) pointers and are
 *     bit-identical to the reference's CPU ring allreduce;
 *   - comm::ICommunicator's collectives are real virtual calls (the
 *     reference's are non-virtual no-ops, include/comm/communicator.h:92-108);
 *   - failures abort with a message, like the reference's CHECK_F;
 *   - custom reducers (ICommunicator::Allreduce(Buffer, ReduceFunction),
 *     Reducer<DType, freduce>, SerializeReducer<DType>) run the user's HOST
 *     function: the inputs move over the device path (allgather), then every
 *     rank folds its own Split chunk in the ring's order (or the whole buffer
 *     in the tree's order at <= rdc_reduce_ring_mincount bytes), calling
 *     reducer(src, dst) exactly as TryReduceScatterRing / TryReduceTree would
 *     (communicator_collective.cc:14-43,115-182), and the chunks are
 *     allgathered.  (The reference declares these; its Reducer /
 *     SerializeReducer::Allreduce call themselves, rdc-inl.h:187-196.)
 * Link with -lrdc_amd.  Header-only otherwise.
 */
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "rdc_amd.h"

namespace rdc {

/*! \brief name of the default communicator (include/comm/communicator.h:21) */
static const std::string kMainCommName = "main";

/*! \brief a (value, index) pair for op::MaxLoc / op::MinLoc (MI355X addition;
 *  MPI_FLOAT_INT / MPI_2INT): "which rank holds the best candidate, and where".
 *  V = float or int32_t: 8 bytes, 8-byte aligned, an int32_t index (the library
 *  refuses a pair buffer that is only 4-byte aligned).
 *  V = double or int64_t: 16 bytes, 16-byte aligned, an int64_t index — the
 *  index type follows the value's width, so it can number every element the
 *  library can move (dtypes 16 / 17; the library refuses a buffer of them that
 *  is only 8-byte aligned).  There is no padded { double, int32 } pair
 *  (MPI_DOUBLE_INT: its padding bytes have no defined bits) and no
 *  { float, int64 } pair. */
template <typename V>
struct alignas(8) ValueIndex {
    static_assert(std::is_same<V, float>::value || std::is_same<V, int32_t>::value,
                  "rdc::ValueIndex<V>: V is float, int32_t, double or int64_t");
    V value;
    int32_t index;
};
template <>
struct alignas(16) ValueIndex<double> {
    double value;
    int64_t index;
};
template <>
struct alignas(16) ValueIndex<int64_t> {
    int64_t value;
    int64_t index;
};
static_assert(sizeof(ValueIndex<double>) == 16 && alignof(ValueIndex<double>) == 16 &&
                  std::is_trivially_copyable<ValueIndex<double>>::value,
              "rdc::ValueIndex<double> is the 16-byte element of dtype 16");
static_assert(sizeof(ValueIndex<int64_t>) == 16 && alignof(ValueIndex<int64_t>) == 16 &&
                  std::is_trivially_copyable<ValueIndex<int64_t>>::value,
              "rdc::ValueIndex<int64_t> is the 16-byte element of dtype 17");
static_assert(sizeof(ValueIndex<float>) == 8 && alignof(ValueIndex<float>) == 8 &&
                  std::is_trivially_copyable<ValueIndex<float>>::value,
              "rdc::ValueIndex<float> is the 8-byte element of dtype 12");
static_assert(sizeof(ValueIndex<int32_t>) == 8 && alignof(ValueIndex<int32_t>) == 8 &&
                  std::is_trivially_copyable<ValueIndex<int32_t>>::value,
              "rdc::ValueIndex<int32_t> is the 8-byte element of dtype 13");

namespace mpi {
/*! \brief reduction operators (include/core/mpi.h:12-17) */
enum OpType {
    kMax = 0,
    kMin = 1,
    kSum = 2,
    kBitwiseOR = 3,
    /*! \brief MI355X additions (MPI_MAXLOC / MPI_MINLOC) over ValueIndex<V> */
    kMaxLoc = 4,
    kMinLoc = 5,
    /*! \brief MI355X additions (MPI_PROD / MPI_BAND / MPI_BXOR); 6 and 7 are unassigned */
    kProd = 8,
    kBitwiseAND = 9,
    kBitwiseXOR = 10
};
/*! \brief element types (include/core/mpi.h:19-30) */
enum DataType {
    kChar = 0,
    kUChar = 1,
    kInt = 2,
    kUInt = 3,
    kLong = 4,
    kULong = 5,
    kFloat = 6,
    kDouble = 7,
    kLongLong = 8,
    kULongLong = 9,
    /*! \brief MI355X additions: rdc::Float16 / rdc::BFloat16 (AllreduceAcc32 and its siblings) */
    kFloat16 = 10,
    kBFloat16 = 11,
    /*! \brief MI355X additions: ValueIndex<float>, ValueIndex<int32_t> (MPI_FLOAT_INT / MPI_2INT) */
    kFloatInt = 12,
    kIntInt = 13,
    /*! \brief ValueIndex<double>, ValueIndex<int64_t>: 16-byte pairs (14 and 15 are unassigned) */
    kDoubleInt64 = 16,
    kInt64Int64 = 17
};
template <typename DType>
inline DataType GetType(void);
template <> inline DataType GetType<char>(void) { return kChar; }
template <> inline DataType GetType<signed char>(void) { return kChar; }
template <> inline DataType GetType<unsigned char>(void) { return kUChar; }
template <> inline DataType GetType<int>(void) { return kInt; }
template <> inline DataType GetType<unsigned int>(void) { return kUInt; }
template <> inline DataType GetType<long>(void) { return kLong; }                       // NOLINT
template <> inline DataType GetType<unsigned long>(void) { return kULong; }             // NOLINT
template <> inline DataType GetType<float>(void) { return kFloat; }
template <> inline DataType GetType<double>(void) { return kDouble; }
template <> inline DataType GetType<long long>(void) { return kLongLong; }              // NOLINT
template <> inline DataType GetType<unsigned long long>(void) { return kULongLong; }    // NOLINT
template <> inline DataType GetType<ValueIndex<float>>(void) { return kFloatInt; }
template <> inline DataType GetType<ValueIndex<int32_t>>(void) { return kIntInt; }
template <> inline DataType GetType<ValueIndex<double>>(void) { return kDoubleInt64; }
template <> inline DataType GetType<ValueIndex<int64_t>>(void) { return kInt64Int64; }
}  // namespace mpi

/*! \brief 16-bit floating elements as storage (IEEE binary16 / bfloat16 bit
 *  patterns; the host header does no arithmetic on them): the element types
 *  of AllreduceAcc32 / ReduceScatterAcc32 / ReduceToAcc32.  A compiler's own
 *  16-bit type of the same layout can be passed through a pointer cast */
struct Float16 {
    uint16_t bits;
};
struct BFloat16 {
    uint16_t bits;
};
static_assert(sizeof(Float16) == 2 && sizeof(BFloat16) == 2, "16-bit elements of dtypes 10 / 11");

namespace detail {
/*! \brief the element types the float32-accumulated Sum takes: anything else
 *  (AllreduceAcc32<float>) does not compile */
template <typename T> struct Acc32Type;
template <> struct Acc32Type<Float16> { static const mpi::DataType kType = mpi::kFloat16; };
template <> struct Acc32Type<BFloat16> { static const mpi::DataType kType = mpi::kBFloat16; };
/*! \brief the element types Avg takes (float, double, rdc::Float16,
 *  rdc::BFloat16): anything else (AllreduceAvg<int>) does not compile */
template <typename T> struct AvgType;
template <> struct AvgType<float> { static const mpi::DataType kType = mpi::kFloat; };
template <> struct AvgType<double> { static const mpi::DataType kType = mpi::kDouble; };
template <> struct AvgType<Float16> { static const mpi::DataType kType = mpi::kFloat16; };
template <> struct AvgType<BFloat16> { static const mpi::DataType kType = mpi::kBFloat16; };
template <typename T> struct IsValueIndex : std::false_type {};
template <typename V> struct IsValueIndex<ValueIndex<V>> : std::true_type {};
/*! \brief MaxLoc / MinLoc fold ValueIndex<V> and nothing else folds it: a
 *  mismatch (Allreduce<op::Sum, ValueIndex<float>>, Allreduce<op::MaxLoc,
 *  float>) does not compile */
template <typename OP, typename DType> struct CheckOpType {
    static const bool kLoc = OP::kType == mpi::kMaxLoc || OP::kType == mpi::kMinLoc;
    static_assert(kLoc == IsValueIndex<DType>::value,
                  "rdc: op::MaxLoc / op::MinLoc go with rdc::ValueIndex<V> elements, and only they do");
    static const bool value = true;
};
}  // namespace detail

/*! \brief reduction operators (include/core/mpi.h:84-120).  kType names the
 *  device kernel the typed collectives launch; Reduce(dst, src) is the
 *  element rule that kernel applies (rdc_amd/csrc/rdc_device.h OpF), kept
 *  here on the host so code written against the reference — its reducer
 *  lambda `op::Reducer<OP,DType>(src.addr(), dst.addr(), src.Count())`
 *  (include/core/rdc-inl.h:130-132) — compiles and folds the same bits. */
namespace op {
struct Max {
    static const mpi::OpType kType = mpi::kMax;
    /*! \brief dst = src when dst < src (a NaN dst stays, a NaN src is ignored) */
    template <typename DType> inline static void Reduce(DType& dst, const DType& src) {  // NOLINT(*)
        if (dst < src) dst = src;
    }
};
struct Min {
    static const mpi::OpType kType = mpi::kMin;
    /*! \brief dst = src when dst > src */
    template <typename DType> inline static void Reduce(DType& dst, const DType& src) {  // NOLINT(*)
        if (dst > src) dst = src;
    }
};
struct Sum {
    static const mpi::OpType kType = mpi::kSum;
    template <typename DType> inline static void Reduce(DType& dst, const DType& src) {  // NOLINT(*)
        dst += src;
    }
};
struct BitOR {
    static const mpi::OpType kType = mpi::kBitwiseOR;
    template <typename DType> inline static void Reduce(DType& dst, const DType& src) {  // NOLINT(*)
        dst |= src;
    }
};
/*! \brief MI355X addition (MPI_PROD): dst = dst * src.  Integers wrap modulo
 *  2^bits: the product is taken on the unsigned type (a signed `dst *= src`
 *  is undefined on overflow), which gives the device kernel's bits.  float and
 *  double: one IEEE multiply, round-to-nearest-even, subnormals kept (build
 *  host code without fast-math or flush-to-zero for equal bits). */
struct Prod {
    static const mpi::OpType kType = mpi::kProd;
    template <typename DType>
    inline static typename std::enable_if<std::is_integral<DType>::value>::type
    Reduce(DType& dst, const DType& src) {  // NOLINT(*)
        typedef typename std::make_unsigned<DType>::type U;
        // unsigned int at the least: narrower types would promote to (signed) int
        typedef typename std::conditional<(sizeof(U) < sizeof(unsigned)), unsigned, U>::type W;
        dst = static_cast<DType>(static_cast<U>(static_cast<W>(static_cast<U>(dst)) * static_cast<W>(static_cast<U>(src))));
    }
    template <typename DType>
    inline static typename std::enable_if<std::is_floating_point<DType>::value>::type
    Reduce(DType& dst, const DType& src) {  // NOLINT(*)
        dst *= src;
    }
};
/*! \brief MI355X additions (MPI_BAND / MPI_BXOR): integer types only, as
 *  BitOR (they do not compile for float or double) */
struct BitAND {
    static const mpi::OpType kType = mpi::kBitwiseAND;
    template <typename DType> inline static void Reduce(DType& dst, const DType& src) {  // NOLINT(*)
        dst &= src;
    }
};
struct BitXOR {
    static const mpi::OpType kType = mpi::kBitwiseXOR;
    template <typename DType> inline static void Reduce(DType& dst, const DType& src) {  // NOLINT(*)
        dst ^= src;
    }
};
/*! \brief MI355X additions (MPI_MAXLOC / MPI_MINLOC) over ValueIndex<V>:
 *  dst = src when dst.value < src.value (MinLoc: >), or when the values are
 *  equal and src.index < dst.index.  So a NaN in dst.value stays and a NaN in
 *  src.value is ignored, as for Max / Min; -0.0f == +0.0f is a tie in value
 *  and the lower index wins; on a full tie (equal value, equal index) dst
 *  stays whole, value bits included, so a +0 / -0 pair with equal indexes
 *  depends on the operand order, as NaN does for Max. */
struct MaxLoc {
    static const mpi::OpType kType = mpi::kMaxLoc;
    template <typename V> inline static void Reduce(ValueIndex<V>& dst, const ValueIndex<V>& src) {  // NOLINT(*)
        if (dst.value < src.value || (dst.value == src.value && src.index < dst.index)) dst = src;
    }
};
struct MinLoc {
    static const mpi::OpType kType = mpi::kMinLoc;
    template <typename V> inline static void Reduce(ValueIndex<V>& dst, const ValueIndex<V>& src) {  // NOLINT(*)
        if (dst.value > src.value || (dst.value == src.value && src.index < dst.index)) dst = src;
    }
};
/*! \brief dst[i] = OP::Reduce(dst[i], src[i]) for i < len, on HOST memory, in
 *  index order (include/core/mpi.h:113-120).  Device buffers: RdcReduce, the
 *  same rule as a HIP kernel. */
template <typename OP, typename DType>
inline void Reducer(const void* src_, void* dst_, uint64_t len) {
    const DType* src = static_cast<const DType*>(src_);
    DType* dst = static_cast<DType*>(dst_);
    for (uint64_t i = 0; i < len; ++i) OP::Reduce(dst[i], src[i]);
}
}  // namespace op


/*! \brief a typed view of memory (include/transport/buffer.h:15-257): address,
 *  size in bytes, optional item size (Count()), byte offsets start/end of a
 *  Slice relative to its parent.  A view, never an owner — except through
 *  AllocTemp/FreeTemp or Alloc/Free (host memory).  Host or device memory.
 *  The reference's RDMA / shm registration and its memory pool are not part
 *  of this path; `pinned` is kept as a flag (RdcNewBuffer pins page-aligned
 *  host ranges for point-to-point). */
class Buffer {
public:
    Buffer() {}
    explicit Buffer(uint64_t size_in_bytes) : size_in_bytes_(size_in_bytes), end_(size_in_bytes) {}
    Buffer(void* addr, uint64_t size_in_bytes) : Buffer(addr, size_in_bytes, 0, size_in_bytes, false) {}
    Buffer(const void* addr, uint64_t size_in_bytes) : Buffer(addr, size_in_bytes, 0, size_in_bytes, false) {}
    Buffer(void* addr, uint64_t size_in_bytes, const bool& pinned)
        : Buffer(addr, size_in_bytes, 0, size_in_bytes, pinned) {}
    Buffer(const void* addr, uint64_t size_in_bytes, const bool& pinned)
        : Buffer(addr, size_in_bytes, 0, size_in_bytes, pinned) {}
    Buffer(void* addr, uint64_t size_in_bytes, uint64_t start, uint64_t end)
        : Buffer(addr, size_in_bytes, start, end, false) {}
    Buffer(const void* addr, uint64_t size_in_bytes, uint64_t start, uint64_t end)
        : Buffer(addr, size_in_bytes, start, end, false) {}
    Buffer(void* addr, uint64_t size_in_bytes, uint64_t start, uint64_t end, const bool& pinned)
        : addr_(addr), size_in_bytes_(size_in_bytes), is_mutable_(true), start_(start), end_(end), pinned_(pinned) {}
    Buffer(const void* addr, uint64_t size_in_bytes, uint64_t start, uint64_t end, const bool& pinned)
        : addr_(const_cast<void*>(addr)), size_in_bytes_(size_in_bytes), is_mutable_(false), start_(start),
          end_(end), pinned_(pinned) {}

    /*! \brief bytes [start, end) of this buffer, same item size (buffer.h:112-119) */
    Buffer Slice(const uint64_t& start, const uint64_t& end) const {
        Buffer b(static_cast<void*>(static_cast<int8_t*>(addr_) + start), end - start, start, end, pinned_);
        b.with_type_ = with_type_;
        b.item_size_ = item_size_;
        b.dtype_ = dtype_;
        b.is_mutable_ = is_mutable_;
        return b;
    }
    template <typename DType> DType* As() const { return reinterpret_cast<DType*>(addr_); }
    template <typename DType> DType* At(const uint32_t& index) { return reinterpret_cast<DType*>(addr_) + index; }
    void* addr() const { return addr_; }
    void set_addr(void* addr) { addr_ = addr; is_mutable_ = true; }
    void set_addr(const void* addr) { addr_ = const_cast<void*>(addr); is_mutable_ = false; }
    uint64_t size_in_bytes() const { return size_in_bytes_; }
    void set_size_in_bytes(const uint64_t& size_in_bytes) { size_in_bytes_ = size_in_bytes; }
    bool is_mutable() const { return is_mutable_; }
    void set_is_mutable(const bool& is_mutable) { is_mutable_ = is_mutable; }
    bool pinned() const { return pinned_; }
    /*! \brief number of items; needs an item size that divides the size (buffer.h:171-174) */
    uint64_t Count() const {
        if (!with_type_ || item_size_ == 0 || size_in_bytes_ % item_size_ != 0) {
            fprintf(stderr, "rdc: Buffer::Count needs an item size dividing the buffer (size %llu, item %llu)\n",
                    (unsigned long long)size_in_bytes_, (unsigned long long)item_size_);
            abort();
        }
        return size_in_bytes_ / item_size_;
    }
    bool with_type() const { return with_type_; }
    void set_with_type(const bool& with_type) { with_type_ = with_type; }
    uint64_t item_size() const { return item_size_; }
    void set_item_size(const uint64_t& item_size) { with_type_ = true; item_size_ = item_size; }
    uint64_t start() const { return start_; }
    uint64_t end() const { return end_; }
    void set_start(const uint64_t start) { start_ = start; }
    void set_end(const uint64_t end) { end_ = end; }
    /*! \brief MI355X addition: the element type, so Allreduce<OP>(Buffer&) can
     *  pick the device kernel (sets the item size too).  -1 = untyped. */
    template <typename DType> void set_type();
    int dtype() const { return dtype_; }
    void AllocTemp(const std::function<void*(const uint64_t&)>& alloc_func) {
        own_data_ = true;
        addr_ = alloc_func(size_in_bytes_);
        is_mutable_ = true;
    }
    void FreeTemp(const std::function<void(void*)>& free_func) {
        own_data_ = false;
        free_func(addr_);
        addr_ = nullptr;
    }
    /*! \brief host memory of size_in_bytes (the reference's pool, buffer.h:220-230) */
    void Alloc() {
        own_data_ = true;
        addr_ = malloc(size_in_bytes_ ? size_in_bytes_ : 1);
        is_mutable_ = true;
    }
    void Free() {
        own_data_ = false;
        free(addr_);
        addr_ = nullptr;
    }

private:
    void* addr_ = nullptr;
    uint64_t size_in_bytes_ = 0;
    bool is_mutable_ = true;
    bool with_type_ = false;
    uint64_t item_size_ = 0;
    int dtype_ = -1;
    bool own_data_ = false;
    uint64_t start_ = 0;
    uint64_t end_ = 0;
    bool pinned_ = false;
};

/*! \brief serialization streams for SerializeReducer (include/io/io.h:14-70,
 *  include/io/memory_io.h:4-32) */
class Stream {
public:
    virtual ~Stream() {}
    virtual size_t Read(void* ptr, size_t size) = 0;
    virtual void Write(const void* ptr, size_t size) = 0;
    template <typename T> void Write(const T& data) {
        static_assert(std::is_trivially_copyable<T>::value, "rdc::Stream::Write<T>: trivially copyable T only");
        Write(&data, sizeof(T));
    }
    template <typename T> bool Read(T* out) {
        static_assert(std::is_trivially_copyable<T>::value, "rdc::Stream::Read<T>: trivially copyable T only");
        return Read(out, sizeof(T)) == sizeof(T);
    }
};
class SeekStream : public Stream {
public:
    virtual void Seek(size_t pos) = 0;
    virtual size_t Tell() = 0;
};
/*! \brief a fixed-size memory region as a stream; writing past the end aborts */
class MemoryFixedSizeStream : public SeekStream {
public:
    MemoryFixedSizeStream(void* p_buffer, size_t buffer_size)
        : p_buffer_(static_cast<char*>(p_buffer)), buffer_size_(buffer_size) {}
    size_t Read(void* ptr, size_t size) override {
        const size_t n = curr_ptr_ + size <= buffer_size_ ? size : buffer_size_ - curr_ptr_;
        if (n) memcpy(ptr, p_buffer_ + curr_ptr_, n);
        curr_ptr_ += n;
        return n;
    }
    void Write(const void* ptr, size_t size) override {
        if (curr_ptr_ + size > buffer_size_) {
            fprintf(stderr, "rdc: MemoryFixedSizeStream: writing %zu bytes past a %zu-byte buffer\n", size,
                    buffer_size_);
            abort();
        }
        if (size) memcpy(p_buffer_ + curr_ptr_, ptr, size);
        curr_ptr_ += size;
    }
    using Stream::Read;
    using Stream::Write;
    void Seek(size_t pos) override { curr_ptr_ = pos; }
    size_t Tell() override { return curr_ptr_; }
    bool AtEnd() const { return curr_ptr_ == buffer_size_; }
    void* inner_buffer() const { return p_buffer_; }
    size_t inner_buffer_size() const { return buffer_size_; }

private:
    char* p_buffer_;
    size_t buffer_size_;
    size_t curr_ptr_ = 0;
};

template <typename DType> inline void Buffer::set_type() {
    set_item_size(sizeof(DType));
    dtype_ = (int)mpi::GetType<DType>();
}

namespace detail {
inline void Check(int rc, const char* what) {
    if (rc != 0) {
        fprintf(stderr, "rdc: %s failed: %s\n", what, RdcGetLastError());
        abort();
    }
}
inline void Fail(const char* what, const std::string& why) {
    fprintf(stderr, "rdc: %s failed: %s\n", what, why.c_str());
    abort();
}
}  // namespace detail

/*! \brief completion of an ISend / IRecv (include/core/work_request.h:240-270).
 *  Owned by the caller; deleting a pending completion is safe. */
class WorkCompletion {
public:
    explicit WorkCompletion(void* h) : h_(h) {}
    ~WorkCompletion() { RdcDelWorkCompletion(h_); }
    WorkCompletion(const WorkCompletion&) = delete;
    WorkCompletion& operator=(const WorkCompletion&) = delete;
    /*! \brief block until done; true on success (the reference's Wait) */
    bool Wait() { return RdcWorkCompletionWait(h_) == 0; }
    /*! \brief WorkStatus bits: 2 pending, 8 finished, 64 error */
    int Status() const { return RdcWorkCompletionStatus(h_); }
    std::string Error() const { return RdcWorkCompletionError(h_); }

private:
    void* h_;
};

namespace comm {
/*! \brief reducer over a received chunk and this rank's chunk, dst = OP(dst, src)
 *  (include/comm/communicator.h:36) */
using ReduceFunction = std::function<void(Buffer src, Buffer dst)>;

/*! \brief a named communicator (include/comm/communicator.h:41-146) */
class ICommunicator {
public:
    ICommunicator(void* handle, const std::string& name) : handle_(handle), name_(name) {}
    virtual ~ICommunicator() {}
    /*! \brief in-place allreduce of count elements (host or device memory) */
    virtual void Allreduce(void* sendrecvbuf, uint64_t count, mpi::DataType dtype, mpi::OpType op) {
        detail::Check(RdcAllreduceOn(handle_, sendrecvbuf, count, (int)dtype, (int)op), "Allreduce");
    }
    /*! \brief in-place reduce-scatter of count elements (host or device memory):
     *  TryReduceScatterRing (communicator_base.h:217-233, "after the function,
     *  node k get k-th segment of the reduction result"; communicator_collective.cc:
     *  115-182).  Chunk GetRank() of utils::Split(0, count, n) receives the
     *  reduction, with Allreduce's bits (the ring order at every size); every
     *  other byte of sendrecvbuf stays as passed */
    virtual void ReduceScatter(void* sendrecvbuf, uint64_t count, mpi::DataType dtype, mpi::OpType op) {
        detail::Check(RdcReduceScatterOn(handle_, sendrecvbuf, count, (int)dtype, (int)op), "ReduceScatter");
    }
    /*! \brief in-place reduction of count elements to rank root (host or device
     *  memory; MPI_Reduce): on root sendrecvbuf receives the reduction, with
     *  Allreduce's bits (the ring order at every size); on every other rank it
     *  is only read.  root must be the same on every rank */
    virtual void ReduceTo(void* sendrecvbuf, uint64_t count, mpi::DataType dtype, mpi::OpType op, int root) {
        detail::Check(RdcReduceToOn(handle_, sendrecvbuf, count, (int)dtype, (int)op, root), "ReduceTo");
    }
    /*! \brief Sum of count kFloat16 / kBFloat16 elements with a float32
     *  accumulator and one rounding (include/rdc_amd.h RdcAllreduceAcc32: the
     *  rule), as Allreduce / ReduceScatter / ReduceTo: the same chunks, the
     *  same result placement, the same untouched bytes.  Any other dtype fails */
    virtual void AllreduceAcc32(void* sendrecvbuf, uint64_t count, mpi::DataType dtype) {
        detail::Check(RdcAllreduceAcc32On(handle_, sendrecvbuf, count, (int)dtype), "AllreduceAcc32");
    }
    virtual void ReduceScatterAcc32(void* sendrecvbuf, uint64_t count, mpi::DataType dtype) {
        detail::Check(RdcReduceScatterAcc32On(handle_, sendrecvbuf, count, (int)dtype), "ReduceScatterAcc32");
    }
    virtual void ReduceToAcc32(void* sendrecvbuf, uint64_t count, mpi::DataType dtype, int root) {
        detail::Check(RdcReduceToAcc32On(handle_, sendrecvbuf, count, (int)dtype, root), "ReduceToAcc32");
    }
    /*! \brief the mean across ranks of count kFloat / kDouble / kFloat16 /
     *  kBFloat16 elements (include/rdc_amd.h RdcAllreduceAvg: the rule — the
     *  ring-order Sum, in float32 for the 16-bit types, then one division by
     *  the world size before the single rounding), as Allreduce /
     *  ReduceScatter / ReduceTo: the same chunks, the same result placement,
     *  the same untouched bytes.  Any other dtype fails */
    virtual void AllreduceAvg(void* sendrecvbuf, uint64_t count, mpi::DataType dtype) {
        detail::Check(RdcAllreduceAvgOn(handle_, sendrecvbuf, count, (int)dtype), "AllreduceAvg");
    }
    virtual void ReduceScatterAvg(void* sendrecvbuf, uint64_t count, mpi::DataType dtype) {
        detail::Check(RdcReduceScatterAvgOn(handle_, sendrecvbuf, count, (int)dtype), "ReduceScatterAvg");
    }
    virtual void ReduceToAvg(void* sendrecvbuf, uint64_t count, mpi::DataType dtype, int root) {
        detail::Check(RdcReduceToAvgOn(handle_, sendrecvbuf, count, (int)dtype, root), "ReduceToAvg");
    }
    /*! \brief in-place prefix reduction across ranks (host or device memory;
     *  MPI_Scan, exclusive: MPI_Exscan): rank r ends with the left fold of
     *  ranks 0..r (exclusive: 0..r-1, r > 0) in rank order; rank 0's buffer is
     *  only read */
    virtual void Scan(void* sendrecvbuf, uint64_t count, mpi::DataType dtype, mpi::OpType op, bool exclusive) {
        detail::Check(RdcScanOn(handle_, sendrecvbuf, count, (int)dtype, (int)op, exclusive ? 1 : 0),
                      exclusive ? "Exscan" : "Scan");
    }
    /*! \brief allreduce with a custom HOST reducer (communicator.h:92-93, virtual
     *  here).  sendrecvbuf needs an item size (Count()).  Ring order per Split
     *  chunk above rdc_reduce_ring_mincount bytes, the tree's order at or below
     *  (TryAllreduce, communicator_collective.cc:6-13); reducer(src, dst) is
     *  called on chunk-sized Buffers exactly as the reference's ring / tree
     *  would call it.  Data moves over the device path (allgather). */
    virtual void Allreduce(Buffer sendrecvbuf, ReduceFunction reducer);
    /*! \brief bucketed allreduce: Allreduce of every bufs[b] (counts[b] items), fused launches */
    virtual void AllreduceCoalesced(void** bufs, const size_t* counts, int nbuf, mpi::DataType dtype,
                                    mpi::OpType op) {
        detail::Check(RdcAllreduceCoalescedOn(handle_, bufs, counts, nbuf, (int)dtype, (int)op), "AllreduceCoalesced");
    }
    /*! \brief broadcast size bytes from root (host or device memory) */
    virtual void Broadcast(void* sendrecvaddr, uint64_t size, int root) {
        detail::Check(RdcBroadcastOn(handle_, sendrecvaddr, size, root), "Broadcast");
    }
    /*! \brief broadcast a Buffer (communicator.h:100-101, virtual here) */
    virtual void Broadcast(Buffer sendrecvbuf, int root) {
        Broadcast(sendrecvbuf.addr(), sendrecvbuf.size_in_bytes(), root);
    }
    /*! \brief bufs[c] holds sizes[c] bytes; bufs[rank] is this rank's data */
    virtual void Allgather(void** bufs, const size_t* sizes) {
        detail::Check(RdcAllgatherOn(handle_, bufs, sizes), "Allgather");
    }
    /*! \brief Allgather of per-rank Buffers (communicator.h:107-119, virtual here) */
    virtual void Allgather(std::vector<Buffer> sendrecvbufs) {
        std::vector<void*> p(sendrecvbufs.size());
        std::vector<size_t> sz(sendrecvbufs.size());
        for (size_t i = 0; i < p.size(); ++i) {
            p[i] = sendrecvbufs[i].addr();
            sz[i] = sendrecvbufs[i].size_in_bytes();
        }
        Allgather(p.data(), sz.data());
    }
    /*! \brief out-of-place all-to-all, equal split (MI355X addition; host or
     *  device memory): bytes [p * bytes_per_peer, +bytes_per_peer) of send land
     *  at [rank * bytes_per_peer, +bytes_per_peer) of rank p's recv (RdcAlltoall) */
    virtual void Alltoall(const void* send, void* recv, size_t bytes_per_peer) {
        detail::Check(RdcAlltoallOn(handle_, send, recv, bytes_per_peer), "Alltoall");
    }
    /*! \brief all-to-all with per-peer byte offsets and lengths (arrays of
     *  GetWorldSize() entries; MI355X addition): send_len[p] here equals
     *  recv_len[GetRank()] on rank p; one segment is at most RdcPlanAlltoallCap
     *  bytes (RdcAlltoallv) */
    virtual void Alltoallv(const void* send, const size_t* send_off, const size_t* send_len, void* recv,
                           const size_t* recv_off, const size_t* recv_len) {
        detail::Check(RdcAlltoallvOn(handle_, send, send_off, send_len, recv, recv_off, recv_len), "Alltoallv");
    }
    /*! \brief non-blocking point-to-point (communicator.h:69-80); host or device
     *  memory; messages on one (src, dst) pair match in order, equal sizes */
    virtual WorkCompletion* ISend(const void* sendaddr, uint64_t size_in_bytes, int dest) {
        void* wc = nullptr;
        detail::Check(RdcCommISend(&wc, handle_, sendaddr, size_in_bytes, dest, nullptr), "ISend");
        return new WorkCompletion(wc);
    }
    virtual WorkCompletion* IRecv(void* recvaddr, uint64_t size_in_bytes, int src) {
        void* wc = nullptr;
        detail::Check(RdcCommIRecv(&wc, handle_, recvaddr, size_in_bytes, src, nullptr), "IRecv");
        return new WorkCompletion(wc);
    }
    virtual WorkCompletion* ISend(Buffer sendbuf, int dest) {
        return ISend(sendbuf.addr(), sendbuf.size_in_bytes(), dest);
    }
    virtual WorkCompletion* IRecv(Buffer recvbuf, int src) {
        return IRecv(recvbuf.addr(), recvbuf.size_in_bytes(), src);
    }
    /*! \brief blocking point-to-point (communicator.h:56-67); aborts on failure */
    virtual void Send(const void* sendaddr, uint64_t size_in_bytes, int dest) {
        WorkCompletion* w = ISend(sendaddr, size_in_bytes, dest);
        if (!w->Wait()) {
            fprintf(stderr, "rdc: Send failed: %s\n", w->Error().c_str());
            abort();
        }
        delete w;
    }
    virtual void Recv(void* recvaddr, uint64_t size_in_bytes, int src) {
        WorkCompletion* w = IRecv(recvaddr, size_in_bytes, src);
        if (!w->Wait()) {
            fprintf(stderr, "rdc: Recv failed: %s\n", w->Error().c_str());
            abort();
        }
        delete w;
    }
    virtual void Send(Buffer sendbuf, int dest) { Send(sendbuf.addr(), sendbuf.size_in_bytes(), dest); }
    virtual void Recv(Buffer recvbuf, int src) { Recv(recvbuf.addr(), recvbuf.size_in_bytes(), src); }
    /*! \brief sub-communicator over ranks of this one (communicator.h:133-134):
     *  collective over every rank of this communicator; null on non-members */
    std::unique_ptr<ICommunicator> CreateGroup(const std::vector<int>& ranks, const std::string& group_name = "");
    int GetRank() const { return RdcCommRank(handle_); }
    int GetWorldSize() const { return RdcCommSize(handle_); }
    bool IsDistributed() const { return GetWorldSize() > 1; }
    std::string name() const { return name_; }
    void* handle() const { return handle_; }

private:
    void* handle_;
    std::string name_;
};

/*! \brief a CreateGroup communicator: owned by its unique_ptr (destroying it is
 *  collective over the group's members) */
class GroupCommunicator : public ICommunicator {
public:
    using ICommunicator::ICommunicator;
    ~GroupCommunicator() override { RdcCommDestroy(handle()); }  // after Finalize: a no-op error code
};

inline std::unique_ptr<ICommunicator> ICommunicator::CreateGroup(const std::vector<int>& ranks,
                                                                 const std::string& group_name) {
    void* h = nullptr;
    detail::Check(RdcCreateGroup(&h, handle_, ranks.data(), (int)ranks.size(), group_name.c_str()), "CreateGroup");
    if (!h) return std::unique_ptr<ICommunicator>();
    return std::unique_ptr<ICommunicator>(new GroupCommunicator(h, group_name));
}

inline void ICommunicator::Allreduce(Buffer buf, ReduceFunction reducer) {
    const int n = GetWorldSize(), r = GetRank();
    const uint64_t S = buf.size_in_bytes();
    if (n <= 1 || S == 0) return;  // communicator_base.h:133-138
    const uint64_t isz = buf.item_size(), count = buf.Count();
    auto view = [&](std::vector<char>& v, uint64_t off, uint64_t len) {
        Buffer b(v.data() + off, len, off, off + len);
        b.set_item_size(isz);
        return b;
    };
    uint64_t mincount = 1;
    detail::Check(RdcCommGetParam(handle_, "rdc_reduce_ring_mincount", &mincount), "Allreduce");
    if (S <= mincount) {
        // TryAllreduceTree (communicator_collective.cc:14-43,71-78): the fold
        // to rank 0 in the tree's order over whole (small: <= the threshold)
        // buffers, then everyone gets rank 0's bytes
        std::vector<std::vector<char>> in((size_t)n, std::vector<char>((size_t)S));
        detail::Check(RdcMemcpy(in[(size_t)r].data(), buf.addr(), S), "Allreduce input copy");
        std::vector<void*> ptrs((size_t)n);
        std::vector<size_t> sizes((size_t)n, (size_t)S);
        for (int q = 0; q < n; ++q) ptrs[(size_t)q] = in[(size_t)q].data();
        Allgather(ptrs.data(), sizes.data());
        int dst[16], src[16];
        const int k = RdcPlanTree(n, dst, src);
        for (int i = 0; i < k; ++i) reducer(view(in[(size_t)src[i]], 0, S), view(in[(size_t)dst[i]], 0, S));
        detail::Check(RdcMemcpy(buf.addr(), in[0].data(), S), "Allreduce result copy");
        return;
    }
    // TryReduceScatterRing (:115-182): rank r ends with chunk r of
    // utils::Split(0, count, n) = x[r] (+) (x[r+1] (+) ... (+) x[r-1]), each
    // step reducer(src = received partial, dst = this rank's chunk).  Only
    // chunk r of every rank's input is needed for that: rank q sends its
    // chunk c straight to rank c (point-to-point over the device path, all
    // pairs at once), (n-1)/n x S in and out per rank — the reference ring's
    // reduce-scatter traffic — and the host holds S/n per peer, not S.
    std::vector<uint64_t> off((size_t)n), len((size_t)n);
    const uint64_t kq = count / (uint64_t)n, km = count % (uint64_t)n;
    for (int c = 0; c < n; ++c) {
        const uint64_t b = (uint64_t)c * kq + std::min<uint64_t>((uint64_t)c, km);
        const uint64_t e = (uint64_t)(c + 1) * kq + std::min<uint64_t>((uint64_t)(c + 1), km);
        off[(size_t)c] = b * isz;
        len[(size_t)c] = (e - b) * isz;
    }
    const uint64_t o = off[(size_t)r], l = len[(size_t)r];
    std::vector<std::vector<char>> x((size_t)n);  // x[q] = rank q's chunk r
    if (l > 0) {
        for (int q = 0; q < n; ++q) x[(size_t)q].resize((size_t)l);
        detail::Check(RdcMemcpy(x[(size_t)r].data(), static_cast<char*>(buf.addr()) + o, l), "Allreduce input copy");
    }
    std::vector<WorkCompletion*> pending;
    for (int k = 1; k < n; ++k) {
        const int q = (r + k) % n;  // send chunk q to rank q; receive chunk r from rank (r - k)
        const int p = (r - k + n) % n;
        if (len[(size_t)q] > 0) pending.push_back(ISend(static_cast<char*>(buf.addr()) + off[(size_t)q], len[(size_t)q], q));
        if (l > 0) pending.push_back(IRecv(x[(size_t)p].data(), l, p));
    }
    bool ok = true;
    std::string err;
    for (WorkCompletion* w : pending) {
        if (!w->Wait() && ok) {
            ok = false;
            err = w->Error();
        }
        delete w;
    }
    if (!ok) detail::Fail("Allreduce chunk exchange", err);
    if (l > 0) {
        std::vector<char> partial(x[(size_t)((r - 1 + n) % n)]);
        for (int j = 2; j <= n; ++j) {
            std::vector<char>& d = x[(size_t)((r - j + n) % n)];
            Buffer dv(d.data(), l, o, o + l);  // the same Slice(o, o + l) view the full-buffer form passed
            dv.set_item_size(isz);
            reducer(view(partial, 0, l), dv);
            partial.swap(d);  // d (now the new partial) is not needed as an input again
        }
        detail::Check(RdcMemcpy(static_cast<char*>(buf.addr()) + o, partial.data(), l), "Allreduce result copy");
    }
    // TryAllgatherRing (:79-114): chunk c from rank c, in place
    std::vector<void*> cb((size_t)n);
    std::vector<size_t> cs((size_t)n);
    for (int c = 0; c < n; ++c) {
        cb[(size_t)c] = static_cast<char*>(buf.addr()) + off[(size_t)c];
        cs[(size_t)c] = (size_t)len[(size_t)c];
    }
    Allgather(cb.data(), cs.data());
}

inline std::vector<ICommunicator*>& Registry() {
    static std::vector<ICommunicator*> r;
    return r;
}
}  // namespace comm

/*! \brief initialise rdc; argv key=val pairs are parameters (rdc-inl.h:21-23) */
inline void Init(int argc, char** argv) { detail::Check(RdcInit(argc, argv), "Init"); }
inline void Init() { Init(0, nullptr); }

inline comm::ICommunicator* Lookup(const std::string& name) {
    for (comm::ICommunicator* c : comm::Registry())
        if (c->name() == name) return c;
    return nullptr;
}
/*! \brief create (collectively) a communicator (rdc-inl.h:25-27) */
inline comm::ICommunicator* NewCommunicator(const std::string& name) {
    if (comm::ICommunicator* c = Lookup(name)) return c;
    void* h = nullptr;
    detail::Check(RdcNewCommunicator(&h, name.c_str()), "NewCommunicator");
    comm::ICommunicator* c = new comm::ICommunicator(h, name);
    comm::Registry().push_back(c);
    return c;
}
/*! \brief an existing communicator; "main" is created on first use (rdc-inl.h:29-31) */
inline comm::ICommunicator* GetCommunicator(const std::string& name = kMainCommName) {
    if (comm::ICommunicator* c = Lookup(name)) return c;
    void* h = nullptr;
    detail::Check(RdcGetCommunicator(&h, name.c_str()), "GetCommunicator");
    comm::ICommunicator* c = new comm::ICommunicator(h, name);
    comm::Registry().push_back(c);
    return c;
}
namespace comm {
/*! \brief the reference's allreduce glue (src/comm/communicator.cc:24-28): the
 *  named communicator's Allreduce(Buffer, ReduceFunction) with `red` as the
 *  reducer.  dtype / op describe the buffer for the caller's benefit only, as
 *  in the reference (which ignores them); the typed device path is
 *  rdc::Allreduce<OP,DType>. */
inline void Allreduce_(Buffer sendrecvbuf, ReduceFunction red, mpi::DataType dtype, mpi::OpType op,
                       const std::string& name) {
    (void)dtype;
    (void)op;
    GetCommunicator(name)->Allreduce(sendrecvbuf, red);
}
}  // namespace comm

inline void Finalize() {
    for (comm::ICommunicator* c : comm::Registry()) delete c;
    comm::Registry().clear();
    detail::Check(RdcFinalize(), "Finalize");
}
inline int GetRank() { return RdcGetRank(); }
inline int GetWorldSize() { return RdcGetWorldSize(); }
inline bool IsDistributed() { return RdcIsDistributed() != 0; }
inline void TrackerPrint(const std::string& msg) { RdcTrackerPrint(msg.c_str()); }
inline void Barrier() { detail::Check(RdcBarrier(), "Barrier"); }

/*! \brief blocking point-to-point on a communicator (include/api.h:10-11, rdc-inl.h:53-66) */
inline void Send(const void* send_data, uint64_t size, int dest, const std::string& comm_name = kMainCommName) {
    GetCommunicator(comm_name)->Send(send_data, size, dest);
}
inline void Recv(void* recv_data, uint64_t size, int src, const std::string& comm_name = kMainCommName) {
    GetCommunicator(comm_name)->Recv(recv_data, size, src);
}

/*! \brief point-to-point on Buffers (rdc-inl.h:53-58; include/api.h:12-13's
 *  size argument, when given, must not exceed the Buffer and limits the bytes) */
inline void Send(const Buffer& sendbuf, int dest) { GetCommunicator()->Send(sendbuf, dest); }
inline void Recv(Buffer& recvbuf, int src) { GetCommunicator()->Recv(recvbuf, src); }
inline void Send(const Buffer& send_buf, size_t size, int dest) {
    if (size > send_buf.size_in_bytes()) {
        fprintf(stderr, "rdc: Send of %zu bytes from a %llu-byte Buffer\n", size,
                (unsigned long long)send_buf.size_in_bytes());
        abort();
    }
    GetCommunicator()->Send(send_buf.addr(), size, dest);
}
inline void Recv(Buffer& recv_buf, size_t size, int src) {
    if (size > recv_buf.size_in_bytes()) {
        fprintf(stderr, "rdc: Recv of %zu bytes into a %llu-byte Buffer\n", size,
                (unsigned long long)recv_buf.size_in_bytes());
        abort();
    }
    GetCommunicator()->Recv(recv_buf.addr(), size, src);
}

/*! \brief sub-communicator of "main" over `ranks` (include/api.h:124-125):
 *  collective over every rank; null on ranks not in the group */
inline std::unique_ptr<comm::ICommunicator> CreateGroup(const std::vector<int>& ranks,
                                                        const std::string& group_name = "") {
    return GetCommunicator()->CreateGroup(ranks, group_name);
}

/*! \brief in-place allreduce (include/api.h:62-64, rdc-inl.h:125-135) */
template <typename OP, typename DType>
inline void Allreduce(DType* sendrecvbuf, uint64_t count, const std::string& comm_name = kMainCommName) {
    static_assert(detail::CheckOpType<OP, DType>::value, "");
    if (GetWorldSize() == 1 || count == 0) return;  // communicator_base.h:133-138
    GetCommunicator(comm_name)->Allreduce(sendrecvbuf, count, mpi::GetType<DType>(), OP::kType);
}

/*! \brief in-place reduce-scatter (MI355X addition to the public surface: the
 *  reference has it only as a schedule step, Communicator::TryReduceScatterRing,
 *  communicator_collective.cc:115-182).  Returns this rank's element range
 *  [first, second) of utils::Split(0, count, n): on return it holds the
 *  reduction, with the bits Allreduce<OP, DType> puts there; every other
 *  element of sendrecvbuf stays as passed */
template <typename OP, typename DType>
inline std::pair<uint64_t, uint64_t> ReduceScatter(DType* sendrecvbuf, uint64_t count,
                                                   const std::string& comm_name = kMainCommName) {
    static_assert(detail::CheckOpType<OP, DType>::value, "");
    if (GetWorldSize() == 1 || count == 0) return std::pair<uint64_t, uint64_t>(0, count);
    comm::ICommunicator* c = GetCommunicator(comm_name);
    c->ReduceScatter(sendrecvbuf, count, mpi::GetType<DType>(), OP::kType);
    uint64_t lo = 0, hi = 0;
    detail::Check(RdcPlanSplit(count, c->GetWorldSize(), c->GetRank(), &lo, &hi), "ReduceScatter");
    return std::pair<uint64_t, uint64_t>(lo, hi);
}

/*! \brief in-place reduction to rank root (MI355X addition to the public
 *  surface; MPI_Reduce.  rdc::Reduce names nothing here, but the C ABI's
 *  RdcReduce is the local element-wise reduce, hence ReduceTo).  On root all
 *  count elements of sendrecvbuf receive the reduction, with the bits
 *  Allreduce<OP, DType> puts there by the ring order, at every size; on every
 *  other rank sendrecvbuf stays exactly as passed.  root must be the same on
 *  every rank; a root outside [0, GetWorldSize()) fails before anything is
 *  launched */
template <typename OP, typename DType>
inline void ReduceTo(DType* sendrecvbuf, uint64_t count, int root, const std::string& comm_name = kMainCommName) {
    static_assert(detail::CheckOpType<OP, DType>::value, "");
    GetCommunicator(comm_name)->ReduceTo(sendrecvbuf, count, mpi::GetType<DType>(), OP::kType, root);
}

/*! \brief in-place Sum of 16-bit floating elements (rdc::Float16 /
 *  rdc::BFloat16) with a float32 accumulator (MI355X addition; the rule:
 *  include/rdc_amd.h RdcAllreduceAcc32).  Allreduce<op::Sum> on such elements
 *  would round to 16 bits at every hop; here the owner of a chunk adds the n
 *  contributions in binary32, in the ring order, and rounds once.  At two
 *  ranks the bits are the ordinary Sum's */
template <typename DType>
inline void AllreduceAcc32(DType* sendrecvbuf, uint64_t count, const std::string& comm_name = kMainCommName) {
    if (GetWorldSize() == 1 || count == 0) return;  // as Allreduce
    GetCommunicator(comm_name)->AllreduceAcc32(sendrecvbuf, count, detail::Acc32Type<DType>::kType);
}

/*! \brief ReduceScatter's float32-accumulated Sum: returns this rank's element
 *  range [first, second) of utils::Split(0, count, n), which holds
 *  AllreduceAcc32's bits on return; every other element stays as passed */
template <typename DType>
inline std::pair<uint64_t, uint64_t> ReduceScatterAcc32(DType* sendrecvbuf, uint64_t count,
                                                        const std::string& comm_name = kMainCommName) {
    const mpi::DataType dt = detail::Acc32Type<DType>::kType;
    if (GetWorldSize() == 1 || count == 0) return std::pair<uint64_t, uint64_t>(0, count);
    comm::ICommunicator* c = GetCommunicator(comm_name);
    c->ReduceScatterAcc32(sendrecvbuf, count, dt);
    uint64_t lo = 0, hi = 0;
    detail::Check(RdcPlanSplit(count, c->GetWorldSize(), c->GetRank(), &lo, &hi), "ReduceScatterAcc32");
    return std::pair<uint64_t, uint64_t>(lo, hi);
}

/*! \brief ReduceTo's float32-accumulated Sum: root receives AllreduceAcc32's
 *  bits, every other rank's buffer stays exactly as passed; a root outside
 *  [0, GetWorldSize()) fails before anything is launched */
template <typename DType>
inline void ReduceToAcc32(DType* sendrecvbuf, uint64_t count, int root, const std::string& comm_name = kMainCommName) {
    GetCommunicator(comm_name)->ReduceToAcc32(sendrecvbuf, count, detail::Acc32Type<DType>::kType, root);
}

/*! \brief in-place mean across ranks of float, double, rdc::Float16 or
 *  rdc::BFloat16 elements (MI355X addition; the rule: include/rdc_amd.h
 *  RdcAllreduceAvg).  Allreduce<op::Sum> followed by a division is a second
 *  pass, rounds 16-bit results twice and cannot undo a float16 sum that
 *  overflowed; here the owner of a chunk divides its ring-order sum (a
 *  float32 sum for the 16-bit types) by the world size before it stores.  At
 *  world size 1 or count 0 the buffer is unchanged */
template <typename DType>
inline void AllreduceAvg(DType* sendrecvbuf, uint64_t count, const std::string& comm_name = kMainCommName) {
    const mpi::DataType dt = detail::AvgType<DType>::kType;
    if (GetWorldSize() == 1 || count == 0) return;  // as Allreduce
    GetCommunicator(comm_name)->AllreduceAvg(sendrecvbuf, count, dt);
}

/*! \brief ReduceScatter's mean: returns this rank's element range [first,
 *  second) of utils::Split(0, count, n), which holds AllreduceAvg's bits on
 *  return; every other element stays as passed */
template <typename DType>
inline std::pair<uint64_t, uint64_t> ReduceScatterAvg(DType* sendrecvbuf, uint64_t count,
                                                      const std::string& comm_name = kMainCommName) {
    const mpi::DataType dt = detail::AvgType<DType>::kType;
    if (GetWorldSize() == 1 || count == 0) return std::pair<uint64_t, uint64_t>(0, count);
    comm::ICommunicator* c = GetCommunicator(comm_name);
    c->ReduceScatterAvg(sendrecvbuf, count, dt);
    uint64_t lo = 0, hi = 0;
    detail::Check(RdcPlanSplit(count, c->GetWorldSize(), c->GetRank(), &lo, &hi), "ReduceScatterAvg");
    return std::pair<uint64_t, uint64_t>(lo, hi);
}

/*! \brief ReduceTo's mean: root receives AllreduceAvg's bits, every other
 *  rank's buffer stays exactly as passed; a root outside [0, GetWorldSize())
 *  fails before anything is launched */
template <typename DType>
inline void ReduceToAvg(DType* sendrecvbuf, uint64_t count, int root, const std::string& comm_name = kMainCommName) {
    GetCommunicator(comm_name)->ReduceToAvg(sendrecvbuf, count, detail::AvgType<DType>::kType, root);
}

/*! \brief in-place inclusive prefix reduction across ranks (MI355X addition to
 *  the public surface; MPI_Scan).  Rank r ends with y[r], where y[0] = x[0] and
 *  y[q] = OP::Reduce(dst = y[q-1], src = x[q]), element by element; rank 0's
 *  buffer stays exactly as passed.  For a floating-point Sum the last rank's
 *  result does not have Allreduce's ring-order bits */
template <typename OP, typename DType>
inline void Scan(DType* sendrecvbuf, uint64_t count, const std::string& comm_name = kMainCommName) {
    static_assert(detail::CheckOpType<OP, DType>::value, "");
    GetCommunicator(comm_name)->Scan(sendrecvbuf, count, mpi::GetType<DType>(), OP::kType, false);
}

/*! \brief in-place exclusive prefix reduction across ranks (MPI_Exscan): rank
 *  r > 0 ends with Scan's result of rank r-1; rank 0's buffer stays exactly as
 *  passed (MPI leaves it undefined) */
template <typename OP, typename DType>
inline void Exscan(DType* sendrecvbuf, uint64_t count, const std::string& comm_name = kMainCommName) {
    static_assert(detail::CheckOpType<OP, DType>::value, "");
    GetCommunicator(comm_name)->Scan(sendrecvbuf, count, mpi::GetType<DType>(), OP::kType, true);
}

/*! \brief out-of-place all-to-all, equal split (MI355X addition to the public
 *  surface: the reference has no personalised exchange).  Elements
 *  [p * count_per_rank, +count_per_rank) of send land at [r * count_per_rank,
 *  +count_per_rank) of rank p's recv (r = this rank); send and recv hold
 *  GetWorldSize() * count_per_rank elements and must not overlap */
template <typename DType>
inline void Alltoall(const DType* send, DType* recv, uint64_t count_per_rank,
                     const std::string& comm_name = kMainCommName) {
    GetCommunicator(comm_name)->Alltoall(send, recv, count_per_rank * sizeof(DType));
}

/*! \brief all-to-all with per-peer counts and displacements, in elements
 *  (MI355X addition; MPI_Alltoallv's arguments): send_counts[p] elements at
 *  send + send_displs[p] go to rank p, which receives them at recv +
 *  recv_displs[r]; send_counts[p] here equals recv_counts[r] on rank p.  One
 *  segment is at most RdcPlanAlltoallCap bytes: slice larger exchanges */
template <typename DType>
inline void Alltoallv(const DType* send, const uint64_t* send_counts, const uint64_t* send_displs, DType* recv,
                      const uint64_t* recv_counts, const uint64_t* recv_displs,
                      const std::string& comm_name = kMainCommName) {
    comm::ICommunicator* c = GetCommunicator(comm_name);
    const size_t n = (size_t)c->GetWorldSize();
    std::vector<size_t> so(n), sl(n), ro(n), rl(n);
    for (size_t p = 0; p < n; ++p) {
        so[p] = (size_t)send_displs[p] * sizeof(DType);
        sl[p] = (size_t)send_counts[p] * sizeof(DType);
        ro[p] = (size_t)recv_displs[p] * sizeof(DType);
        rl[p] = (size_t)recv_counts[p] * sizeof(DType);
    }
    c->Alltoallv(send, so.data(), sl.data(), recv, ro.data(), rl.data());
}

/*! \brief in-place allreduce of a typed Buffer (include/api.h:65-66; declared
 *  but never defined in the reference): the Buffer must carry its element
 *  type (Buffer::set_type<DType>()), which picks the device kernel */
template <typename OP>
inline void Allreduce(Buffer& sendrecvbuf, const std::string& comm_name = kMainCommName) {
    if (sendrecvbuf.dtype() < 0) {
        fprintf(stderr, "rdc: Allreduce<OP>(Buffer&) needs a typed Buffer (Buffer::set_type<DType>())\n");
        abort();
    }
    if (GetWorldSize() == 1 || sendrecvbuf.size_in_bytes() == 0) return;
    GetCommunicator(comm_name)->Allreduce(sendrecvbuf.addr(), sendrecvbuf.Count(), (mpi::DataType)sendrecvbuf.dtype(),
                                          OP::kType);
}

/*! \brief bucketed allreduce (MI355X addition; test/mallreduce.cc's back-to-back shape):
 *  the result of Allreduce<OP,DType>(bufs[b], counts[b]) for every b, bit-identical,
 *  moved in fused device launches */
template <typename OP, typename DType>
inline void AllreduceCoalesced(DType** bufs, const uint64_t* counts, int nbuf,
                               const std::string& comm_name = kMainCommName) {
    static_assert(detail::CheckOpType<OP, DType>::value, "");
    if (GetWorldSize() == 1 || nbuf == 0) return;
    std::vector<size_t> c((size_t)nbuf);
    for (int b = 0; b < nbuf; ++b) c[(size_t)b] = (size_t)counts[b];
    GetCommunicator(comm_name)->AllreduceCoalesced(reinterpret_cast<void**>(bufs), c.data(), nbuf,
                                                   mpi::GetType<DType>(), OP::kType);
}

/*! \brief broadcast a memory region from root (include/api.h:23-24) */
inline void Broadcast(void* sendrecv_data, uint64_t size, int root, const std::string& comm_name = kMainCommName) {
    if (GetWorldSize() == 1 || size == 0) return;
    GetCommunicator(comm_name)->Broadcast(sendrecv_data, size, root);
}
/*! \brief broadcast a Buffer (include/api.h:25-26, rdc-inl.h:71-75) */
inline void Broadcast(Buffer& buf, int root, const std::string& comm_name = kMainCommName) {
    if (GetWorldSize() == 1 || buf.size_in_bytes() == 0) return;
    GetCommunicator(comm_name)->Broadcast(buf, root);
}
/*! \brief broadcast a vector, resizing receivers (rdc-inl.h:76-88) */
template <typename DType>
inline void Broadcast(std::vector<DType>& sendrecv_data, int root, const std::string& comm_name = kMainCommName) {
    uint64_t size = sendrecv_data.size();
    Broadcast(&size, sizeof(size), root, comm_name);
    if (sendrecv_data.size() != size) sendrecv_data.resize(size);
    if (size != 0) Broadcast(sendrecv_data.data(), size * sizeof(DType), root, comm_name);
}
/*! \brief broadcast a string, resizing receivers (rdc-inl.h:89-100) */
inline void Broadcast(std::string& sendrecv_data, int root, const std::string& comm_name = kMainCommName) {
    uint64_t size = sendrecv_data.length();
    Broadcast(&size, sizeof(size), root, comm_name);
    if (sendrecv_data.length() != size) sendrecv_data.resize(size);
    if (size != 0) Broadcast(&sendrecv_data[0], size, root, comm_name);
}

/*! \brief allgather of per-rank buffers (include/api.h:51-52): sendrecv_data[c]
 *  holds counts[c] items of type_nbytes bytes; this rank's own entry is the input */
inline void Allgather(void** sendrecv_data, size_t type_nbytes, size_t* counts,
                      const std::string& comm_name = kMainCommName) {
    const int n = GetWorldSize();
    if (n == 1) return;
    std::vector<size_t> sizes((size_t)n);
    for (int i = 0; i < n; ++i) sizes[(size_t)i] = counts[i] * type_nbytes;
    GetCommunicator(comm_name)->Allgather(sendrecv_data, sizes.data());
}
/*! \brief allgather of per-rank Buffers (rdc-inl.h:106-110) */
inline void Allgather(std::vector<Buffer>& sendrecvbufs, const std::string& comm_name = kMainCommName) {
    if (GetWorldSize() == 1) return;
    GetCommunicator(comm_name)->Allgather(sendrecvbufs);
}
/*! \brief allgather of pre-sized vectors (include/api.h:47-49, rdc-inl.h:112-122) */
template <typename DType>
inline void Allgather(std::vector<std::vector<DType>>& sendrecv_data, const std::string& comm_name = kMainCommName) {
    const int n = GetWorldSize();
    if (n == 1) return;
    std::vector<void*> bufs((size_t)n);
    std::vector<size_t> sizes((size_t)n);
    for (int i = 0; i < n; ++i) {
        bufs[(size_t)i] = sendrecv_data[(size_t)i].data();
        sizes[(size_t)i] = sendrecv_data[(size_t)i].size() * sizeof(DType);
    }
    GetCommunicator(comm_name)->Allgather(bufs.data(), sizes.data());
}

/*! \brief custom element-wise reduction (include/api.h:135-146): freduce(dst,
 *  src) on every item, as ReducerSafe_ applies it (rdc-inl.h:142-155: items
 *  copied out and back, no alignment assumed).  DType must be trivially
 *  copyable.  Runs on the host (see ICommunicator::Allreduce(Buffer, ...)). */
template <typename DType, void (*freduce)(DType& dst, const DType& src)>  // NOLINT(*)
class Reducer {
public:
    static_assert(std::is_trivially_copyable<DType>::value, "rdc::Reducer needs a trivially copyable DType");
    Reducer() {}
    void Allreduce(DType* sendrecvbuf, size_t count, const std::string& comm_name = kMainCommName) {
        if (GetWorldSize() == 1 || count == 0) return;
        Buffer b(static_cast<void*>(sendrecvbuf), (uint64_t)count * sizeof(DType));
        b.set_item_size(sizeof(DType));
        GetCommunicator(comm_name)->Allreduce(b, [](Buffer src, Buffer dst) {
            const char* ps = static_cast<const char*>(src.addr());
            char* pd = static_cast<char*>(dst.addr());
            for (uint64_t i = 0, n = src.Count(); i < n; ++i) {
                DType td, ts;
                memcpy(&td, pd + i * sizeof(DType), sizeof(DType));
                memcpy(&ts, ps + i * sizeof(DType), sizeof(DType));
                freduce(td, ts);
                memcpy(pd + i * sizeof(DType), &td, sizeof(DType));
            }
        });
    }
};

/*! \brief reduction of serializable objects (include/api.h:147-174): each of
 *  the `count` objects is saved into a max_nbyte slot (DType::Save(Stream&)
 *  const), slots are reduced with DType::Load(Stream&) + DType::Reduce(const
 *  DType& src, size_t max_nbyte) + Save, and loaded back (the closure of
 *  rdc-inl.h:168-184).  Runs on the host like Reducer. */
template <typename DType>
class SerializeReducer {
public:
    SerializeReducer() {}
    void Allreduce(DType* sendrecvobj, size_t max_nbyte, size_t count, const std::string& comm_name = kMainCommName) {
        if (GetWorldSize() == 1 || count == 0) return;
        buffer_.assign(max_nbyte * count, '\0');
        for (size_t i = 0; i < count; ++i) {
            MemoryFixedSizeStream fs(&buffer_[i * max_nbyte], max_nbyte);
            sendrecvobj[i].Save(fs);
        }
        Buffer b(static_cast<void*>(&buffer_[0]), (uint64_t)(max_nbyte * count));
        b.set_item_size(max_nbyte);
        GetCommunicator(comm_name)->Allreduce(b, [max_nbyte](Buffer src, Buffer dst) {
            char* ps = static_cast<char*>(src.addr());
            char* pd = static_cast<char*>(dst.addr());
            for (uint64_t i = 0, n = src.Count(); i < n; ++i) {
                DType tsrc, tdst;
                MemoryFixedSizeStream fsrc(ps + i * max_nbyte, max_nbyte), fdst(pd + i * max_nbyte, max_nbyte);
                tsrc.Load(fsrc);
                tdst.Load(fdst);
                tdst.Reduce(tsrc, max_nbyte);
                fdst.Seek(0);
                tdst.Save(fdst);
            }
        });
        for (size_t i = 0; i < count; ++i) {
            MemoryFixedSizeStream fs(&buffer_[i * max_nbyte], max_nbyte);
            sendrecvobj[i].Load(fs);
        }
    }

private:
    std::string buffer_;  // count slots of max_nbyte bytes
};

}  // namespace rdc
