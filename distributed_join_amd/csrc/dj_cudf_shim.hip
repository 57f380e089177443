/*
 * dj_cudf_shim.hip — cudf::column, the owning device column of
 * include/dj_cudf_types.hpp: pool-backed storage and the lazy null count.
 */
#include "dj_host.hpp"

using namespace dj_host;

namespace cudf {

column::column(data_type type, size_type size) : _type(type), _size(size)
{
  size_t bytes = (size_t)size * size_of(type);
  if (bytes) _data = pool_alloc(bytes);
}

column::column(data_type type, size_type size, void* adopt) : _type(type), _size(size), _data(adopt)
{
}

column::column(size_type size, int64_t chars_bytes)
  : _type(data_type(type_id::STRING)), _size(size), _chars_size(chars_bytes)
{
  _data = pool_alloc(((size_t)size + 1) * sizeof(int32_t));
  /* an empty STRING column is complete as built: offsets = {0} */
  if (size == 0) DJ_HIP_CALL(hipMemset(_data, 0, sizeof(int32_t)));
  if (chars_bytes) _chars = pool_alloc((size_t)chars_bytes);
}

column::column(column&& o) noexcept
  : _type(o._type),
    _size(o._size),
    _data(o._data),
    _chars(o._chars),
    _chars_size(o._chars_size),
    _null_mask(o._null_mask),
    _null_count(o._null_count)
{
  o._data = nullptr;
  o._chars = nullptr;
  o._size = 0;
  o._chars_size = 0;
  o._null_mask = nullptr;
  o._null_count = 0;
}

column& column::operator=(column&& o) noexcept
{
  if (this != &o) {
    if (_data) pool_free(_data);
    if (_chars) pool_free(_chars);
    if (_null_mask) pool_free(_null_mask);
    _type = o._type;
    _size = o._size;
    _data = o._data;
    _chars = o._chars;
    _chars_size = o._chars_size;
    _null_mask = o._null_mask;
    _null_count = o._null_count;
    o._data = nullptr;
    o._chars = nullptr;
    o._size = 0;
    o._chars_size = 0;
    o._null_mask = nullptr;
    o._null_count = 0;
  }
  return *this;
}

column::~column()
{
  if (_data) pool_free(_data);
  if (_chars) pool_free(_chars);
  if (_null_mask) pool_free(_null_mask);
}

void column::set_null_mask(void* adopt, size_type null_count)
{
  if (_null_mask && _null_mask != adopt) pool_free(_null_mask);
  _null_mask = (bitmask_type*)adopt;
  _null_count = adopt ? null_count : 0;
}

bitmask_type* column::allocate_null_mask()
{
  /* never empty, so that a 0-row column can still be nullable() */
  set_null_mask(pool_alloc(std::max<size_t>(bitmask_allocation_size_bytes(_size), 64)),
                UNKNOWN_NULL_COUNT);
  return _null_mask;
}

size_type column::null_count() const
{
  if (_null_count != UNKNOWN_NULL_COUNT) return _null_count;
  if (_null_mask == nullptr || _size == 0) return _null_count = 0;
  hipStream_t st = dj_rt_stream();
  DBuf cnt(8);
  DJ_HIP_CALL(hipMemsetAsync(cnt.p, 0, 8, st));
  dj::count_unset_bits(_null_mask, _size, (unsigned long long*)cnt.p, st);
  return _null_count = (size_type)read_back<unsigned long long>(cnt.p, st);
}

}  // namespace cudf
