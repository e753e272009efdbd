// The part of the DLPack C ABI (dmlc/dlpack, dlpack.h) that
// radler.gpu.DeviceArray exchanges: the unversioned DLManagedTensor behind a
// "dltensor" capsule. Where the build finds PyTorch's copy of the header
// (build.py defines RADLER_HAVE_ATEN_DLPACK), that one is used; elsewhere the
// structs are restated here, so the module builds without torch. The layout
// is frozen by the DLPack specification.
#pragma once

#if defined(RADLER_HAVE_ATEN_DLPACK)
#include <ATen/dlpack.h>
#else

#include <cstdint>

extern "C" {

typedef enum {
  kDLCPU = 1,
  kDLCUDA = 2,
  kDLCUDAHost = 3,
  kDLROCM = 10,
  kDLROCMHost = 11,
} DLDeviceType;

typedef struct {
  DLDeviceType device_type;
  int32_t device_id;
} DLDevice;

typedef enum {
  kDLInt = 0U,
  kDLUInt = 1U,
  kDLFloat = 2U,
  kDLOpaqueHandle = 3U,
  kDLBfloat = 4U,
  kDLComplex = 5U,
  kDLBool = 6U,
} DLDataTypeCode;

typedef struct {
  uint8_t code;
  uint8_t bits;
  uint16_t lanes;
} DLDataType;

typedef struct {
  void* data;
  DLDevice device;
  int32_t ndim;
  DLDataType dtype;
  int64_t* shape;
  int64_t* strides;  // in elements; NULL: compact row-major
  uint64_t byte_offset;
} DLTensor;

typedef struct DLManagedTensor {
  DLTensor dl_tensor;
  void* manager_ctx;
  void (*deleter)(struct DLManagedTensor* self);
} DLManagedTensor;

}  // extern "C"

#endif  // RADLER_HAVE_ATEN_DLPACK

static_assert(sizeof(DLDevice) == 8 && sizeof(DLDataType) == 4, "DLPack ABI");
static_assert(sizeof(void*) != 8 || sizeof(DLTensor) == 48, "DLPack ABI");
