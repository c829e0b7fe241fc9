// gram_sym_kernel, the pass that fills the mirror half of G = R^T R; see gram_sym.hpp
#define SLIM_GRAM_SYM_KERNEL
#include "gram_sym.hpp"
namespace slimamd {
GramSymFn gram_sym_fn() { return gram_sym_kernel; }
}  // namespace slimamd
