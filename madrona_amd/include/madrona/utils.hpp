// Small integer helpers.  API contract: reference include/madrona/utils.hpp
// (divideRoundUp, roundUp, roundUpPow2, int32NextPow2, int32Log2, u32mulhi;
// ArrayQueue :65-90 and copyN / zeroN / fillN :197-206, defined in utils.inl
// :3-53 and :66-86).
#pragma once

#include <madrona/macros.hpp>
#include <madrona/types.hpp>

#include <cstring>
#include <type_traits>

namespace madrona {

// Ring buffer over caller memory (reference utils.hpp:65-90, utils.inl:3-53).
// No overflow check, like the reference: a caller never holds more than
// capacity elements at once (Navmesh::bfsFromPoly visits each polygon once).
template <typename T>
class ArrayQueue {
public:
    MADRONA_HD inline ArrayQueue(T *data, uint32_t capacity)
        : data_(data), capacity_(capacity), head_(0), tail_(0)
    {}

    MADRONA_HD inline void add(T t)
    {
        data_[tail_] = t;
        tail_ = increment(tail_);
    }

    MADRONA_HD inline T remove()
    {
        T t = data_[head_];
        head_ = increment(head_);
        return t;
    }

    MADRONA_HD inline uint32_t capacity() const { return capacity_; }
    MADRONA_HD inline bool isEmpty() const { return head_ == tail_; }

    MADRONA_HD inline void clear()
    {
        head_ = 0;
        tail_ = 0;
    }

private:
    MADRONA_HD inline uint32_t increment(uint32_t i)
    {
        return i == capacity_ - 1 ? 0u : i + 1;
    }

    T *data_;
    uint32_t capacity_;
    uint32_t head_;
    uint32_t tail_;
};

namespace utils {

template <typename T>
MADRONA_HD constexpr inline T divideRoundUp(T a, T b)
{
    return (a + (b - 1)) / b;
}

template <typename T>
MADRONA_HD constexpr inline T roundUp(T offset, T alignment)
{
    return divideRoundUp(offset, alignment) * alignment;
}

// alignment must be a power of two
template <typename T>
MADRONA_HD constexpr inline T roundUpPow2(T offset, T alignment)
{
    return (offset + alignment - 1) & ~(alignment - 1);
}

MADRONA_HD constexpr inline bool isPower2(uint64_t v)
{
    return v != 0 && (v & (v - 1)) == 0;
}

MADRONA_HD constexpr inline uint32_t int32NextPow2(uint32_t v)
{
    if (v <= 1) return 1;
    return 1u << (32 - __builtin_clz(v - 1));
}

MADRONA_HD constexpr inline uint32_t int32Log2(uint32_t v)
{
    return 31u - (uint32_t)__builtin_clz(v);
}

MADRONA_HD constexpr inline uint32_t u32mulhi(uint32_t a, uint32_t b)
{
    return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
}

// Element-wise copy / clear / fill (reference utils.inl:66-86: memcpy, memset
// and a loop).  On the device an element loop: a memcpy of a run-time length
// lowers to a byte loop there.
template <typename T>
MADRONA_HD inline void copyN(std::type_identity_t<T> *dst,
                             const std::type_identity_t<T> *src,
                             CountT num_elems)
{
#if defined(__HIP_DEVICE_COMPILE__)
    for (CountT i = 0; i < num_elems; i++) {
        dst[i] = src[i];
    }
#else
    memcpy(dst, src, sizeof(T) * num_elems);
#endif
}

template <typename T>
MADRONA_HD inline void zeroN(std::type_identity_t<T> *ptr, CountT num_elems)
{
#if defined(__HIP_DEVICE_COMPILE__)
    for (CountT i = 0; i < num_elems; i++) {
        ptr[i] = T {};
    }
#else
    memset(ptr, 0, num_elems * sizeof(T));
#endif
}

template <typename T>
MADRONA_HD inline void fillN(std::type_identity_t<T> *ptr, T v, CountT num_elems)
{
    for (CountT i = 0; i < num_elems; i++) {
        ptr[i] = v;
    }
}

template <typename> struct PackDelegator;
template <template <typename...> typename T, typename... Args>
struct PackDelegator<T<Args...>> {
    template <typename Fn>
    static auto call(Fn &&fn) -> decltype(fn.template operator()<Args...>())
    {
        return fn.template operator()<Args...>();
    }
};

}
}
