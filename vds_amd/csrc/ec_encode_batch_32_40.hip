// ec_encode_batch_32_40.hip -- k_encode_batch<32,40> (ec_encode_batch.hpp): one translation unit per
// shape, as the uniform kernels' ec_encode_32_40.hip.
#include "ec_encode_batch.hpp"

namespace vds_ec {

hipError_t launch_encode_batch_32_40(const EncBatchLaunch &b, hipStream_t s) {
  return launch_encode_batch_shape<32, 40, 5, 8, false>(b, s);
}

}  // namespace vds_ec
