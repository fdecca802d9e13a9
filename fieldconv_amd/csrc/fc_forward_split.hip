// FieldConv forward, split-half MFMA instantiation (kernels: fc_forward_kernels.hpp).
#include "fc_forward_route.hpp"

namespace fc {

template int forward_launch_mode<true>(const float*, const float*, const fc_csr*, const float*, float*, const fc_dims*, int,
                                       const ForwardRoute&, const FwdEpi&, hipStream_t);

}  // namespace fc
