// diaglib_amd/csrc/spmm_transpose_sort.hip -- the stable sort behind dla_spmm_transpose_prepare (hip_engine.hip), in a translation
// unit of its own so that the engine does not compile rocPRIM's headers.  rocprim::radix_sort_pairs is stable (equal keys keep the
// order of the input: the entries of a column stay in the order of the caller's CSR arrays) and header-only: nothing new is linked.
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

namespace dla {

// temp == nullptr: *temp_bytes <- the size of the temporary storage, nothing is launched; else (key_in, val_in) sorted by the low
// key_bits bits of the key into (key_out, val_out), enqueued on st.  The inputs are left as they are.
hipError_t sort_pairs_by_key(void* temp, size_t* temp_bytes, const int* key_in, int* key_out, const int* val_in, int* val_out,
                             size_t count, int key_bits, hipStream_t st)
{
  return rocprim::radix_sort_pairs(temp, *temp_bytes, key_in, key_out, val_in, val_out, count, 0u, (unsigned)key_bits, st);
}

}  // namespace dla
