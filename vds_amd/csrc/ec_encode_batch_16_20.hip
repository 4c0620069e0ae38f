// ec_encode_batch_16_20.hip -- k_encode_batch<16,20> (ec_encode_batch.hpp): one translation unit per
// shape, as the uniform kernels' ec_encode_16_20.hip.
#include "ec_encode_batch.hpp"

namespace vds_ec {

hipError_t launch_encode_batch_16_20(const EncBatchLaunch &b, hipStream_t s) {
  return launch_encode_batch_shape<16, 20, 5, 4, false>(b, s);
}

}  // namespace vds_ec
