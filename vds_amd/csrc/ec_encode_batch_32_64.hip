// ec_encode_batch_32_64.hip -- k_encode_batch<32,64> (ec_encode_batch.hpp): one translation unit per
// shape, as the uniform kernels' ec_encode_32_64.hip.
#include "ec_encode_batch.hpp"

namespace vds_ec {

hipError_t launch_encode_batch_32_64(const EncBatchLaunch &b, hipStream_t s) {
  return launch_encode_batch_shape<32, 64, 8, 8, true>(b, s);
}

}  // namespace vds_ec
