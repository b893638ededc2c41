// TEST INFRASTRUCTURE.  The C++ surface of shape queries (<madrona/mw_gpu.hpp>:
// MWCudaExecutor::makeShapeQuery / setStepShapes, MWHipShapeQuery) named member
// by member.  Included by a plain host translation unit
// (shapes_conformance_host.cpp) and by a HIP one compiled for gfx950
// (shapes_conformance.hip), each with its own SHAPESCONF_NAME; a missing or
// mis-declared member fails the build.  tests/test_shape_query_abi.py.
#include <madrona/mw_gpu.hpp>

#include <mwhip.h>

#include <type_traits>
#include <utility>

static_assert(MWHIP_ABI_VERSION == 9u, "shape queries were added under ABI 9, without a bump");
static_assert(sizeof(mwhip_shapes_desc) == 72, "{ six uint32, three sources }");
static_assert(sizeof(mwhip_shape_plan) == 176 && sizeof(mwhip_shape_args) == 56,
              "what the runtime and the simulator's kernel share");
// (the structs the earlier queries added stay as simulator libraries were
// compiled against them)
static_assert(sizeof(mwhip_ray_source) == 16 && sizeof(mwhip_box_plan) == 104 &&
              sizeof(mwhip_box_args) == 56 && sizeof(mwhip_contact_plan) == 80 &&
              sizeof(mwhip_contact_args) == 56);

namespace {

using madrona::MWCudaExecutor;
using madrona::MWHipShapeQuery;
using madrona::py::Tensor;

static_assert(std::is_same_v<decltype(std::declval<MWCudaExecutor &>().makeShapeQuery(
                                 std::declval<const mwhip_shapes_desc &>())),
                             MWHipShapeQuery>);
static_assert(std::is_same_v<decltype(std::declval<MWCudaExecutor &>().setStepShapes(
                                 std::declval<const MWHipShapeQuery *>(), true)), void>);
static_assert(std::is_same_v<decltype(std::declval<MWHipShapeQuery &>().compute()), void>);
static_assert(std::is_same_v<decltype(std::declval<MWHipShapeQuery &>().computeAsync()), void>);
#define SHAPESCONF_TENSOR(member) \
    static_assert(std::is_same_v< \
        decltype(std::declval<const MWHipShapeQuery &>().member()), Tensor>)
SHAPESCONF_TENSOR(worldsTensor);
SHAPESCONF_TENSOR(excludesTensor);
SHAPESCONF_TENSOR(objectsTensor);
SHAPESCONF_TENSOR(positionsTensor);
SHAPESCONF_TENSOR(rotationsTensor);
SHAPESCONF_TENSOR(scalesTensor);
SHAPESCONF_TENSOR(statusTensor);
SHAPESCONF_TENSOR(countsTensor);
SHAPESCONF_TENSOR(hitsTensor);
SHAPESCONF_TENSOR(shapeIsRefTensor);
SHAPESCONF_TENSOR(numPointsTensor);
SHAPESCONF_TENSOR(normalsTensor);
SHAPESCONF_TENSOR(pointsTensor);
static_assert(std::is_same_v<decltype(std::declval<const MWHipShapeQuery &>().handleSource()),
                             mwhip_gather_source>);
static_assert(std::is_same_v<
    decltype(std::declval<const MWHipShapeQuery &>().numBundles()), uint64_t>);
static_assert(std::is_same_v<
    decltype(std::declval<const MWHipShapeQuery &>().numShapes()), uint64_t>);
static_assert(std::is_same_v<
    decltype(std::declval<const MWHipShapeQuery &>().maxHits()), uint64_t>);
static_assert(std::is_same_v<
    decltype(std::declval<const MWHipShapeQuery &>().handle()), uint64_t>);

}

extern "C" {

#define SHAPESCONF_API __attribute__((visibility("default")))
#define SHAPESCONF_CAT2(a, b) a##b
#define SHAPESCONF_CAT(a, b) SHAPESCONF_CAT2(a, b)

// bit 0: default constructible, 1: not copy constructible, 2: not copy
// assignable, 3: move constructible, 4: move assignable
SHAPESCONF_API uint32_t SHAPESCONF_CAT(SHAPESCONF_NAME, _traits)()
{
    return (std::is_default_constructible_v<MWHipShapeQuery> ? 1u : 0u) |
        (!std::is_copy_constructible_v<MWHipShapeQuery> ? 2u : 0u) |
        (!std::is_copy_assignable_v<MWHipShapeQuery> ? 4u : 0u) |
        (std::is_move_constructible_v<MWHipShapeQuery> ? 8u : 0u) |
        (std::is_move_assignable_v<MWHipShapeQuery> ? 16u : 0u);
}

// the caps, flags and codes of the header, as this translation unit saw them
SHAPESCONF_API uint32_t SHAPESCONF_CAT(SHAPESCONF_NAME, _caps)()
{
    return (uint32_t)MWHIP_MAX_STEP_SHAPES << 16 | (uint32_t)MWHIP_SHAPES_NUM_BUFS << 8 |
        (uint32_t)MWHIP_SHAPES_PLAIN << 4 |
        (uint32_t)(MWHIP_SHAPES_OK - MWHIP_SHAPES_UNSUPPORTED);
}

// every member once, on a caller's executor and a query that owns its world
// and exclude buffers; returns shapes x hits (0: something was not as it should
// be)
SHAPESCONF_API uint64_t SHAPESCONF_CAT(SHAPESCONF_NAME, _cycle)(
    MWCudaExecutor *exec, const mwhip_shapes_desc *desc)
{
    MWHipShapeQuery first = exec->makeShapeQuery(*desc);
    first.compute();
    first.computeAsync();
    exec->setStepShapes(&first, true);
    exec->setStepShapes(&first, false);
    MWHipShapeQuery second(std::move(first));
    MWHipShapeQuery third;
    third = std::move(second);
    const Tensor worlds = third.worldsTensor();
    const Tensor excludes = third.excludesTensor();
    const Tensor objects = third.objectsTensor();
    const Tensor positions = third.positionsTensor();
    const Tensor rotations = third.rotationsTensor();
    const Tensor scales = third.scalesTensor();
    const Tensor status = third.statusTensor();
    const Tensor counts = third.countsTensor();
    const Tensor hits = third.hitsTensor();
    const Tensor is_ref = third.shapeIsRefTensor();
    const Tensor num_points = third.numPointsTensor();
    const Tensor normals = third.normalsTensor();
    const Tensor points = third.pointsTensor();
    const mwhip_gather_source source = third.handleSource();
    const int64_t shapes = (int64_t)third.numShapes(), k = (int64_t)third.maxHits();
    if (third.handle() == 0 || worlds.numDims() != 1 || excludes.numDims() != 2 ||
            objects.numDims() != 1 || positions.numDims() != 2 || rotations.numDims() != 2 ||
            scales.numDims() != 2 || status.numDims() != 1 || counts.numDims() != 1 ||
            hits.numDims() != 3 || is_ref.numDims() != 2 || num_points.numDims() != 2 ||
            normals.numDims() != 3 || points.numDims() != 3 || !status.isOnGPU() ||
            worlds.dims()[0] != (int64_t)third.numBundles() || excludes.dims()[0] != shapes ||
            excludes.dims()[1] != 2 || objects.dims()[0] != shapes ||
            positions.dims()[1] != 3 || rotations.dims()[1] != 4 || scales.dims()[1] != 3 ||
            status.dims()[0] != shapes || counts.dims()[0] != shapes ||
            hits.dims()[0] != shapes || hits.dims()[1] != k || hits.dims()[2] != 2 ||
            is_ref.dims()[1] != k || num_points.dims()[1] != k || normals.dims()[2] != 3 ||
            points.dims()[2] != 16 || source.src != hits.devicePtr() ||
            source.num_records != (uint64_t)shapes * (uint64_t)k || source.record_bytes != 8u ||
            source.handles_per_record != 1u) {
        return 0;
    }
    return (uint64_t)shapes * (uint64_t)k;
}

}
