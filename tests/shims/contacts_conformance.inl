// TEST INFRASTRUCTURE.  The C++ surface of contact queries (<madrona/mw_gpu.hpp>:
// MWCudaExecutor::makeContactQuery / setStepContacts, MWHipContactQuery) named
// member by member.  Included by a plain host translation unit
// (contacts_conformance_host.cpp) and by a HIP one compiled for gfx950
// (contacts_conformance.hip), each with its own CONTACTSCONF_NAME; a missing or
// mis-declared member fails the build.  tests/test_contact_query_abi.py.
#include <madrona/mw_gpu.hpp>

#include <mwhip.h>

#include <type_traits>
#include <utility>

static_assert(MWHIP_ABI_VERSION == 9u, "contact queries were added under ABI 9, without a bump");
static_assert(sizeof(mwhip_contacts_desc) == 32, "{ four uint32, one source }");
static_assert(sizeof(mwhip_contact_plan) == 80 && sizeof(mwhip_contact_args) == 56,
              "what the runtime and the simulator's kernel share");
// (the structs ray and box queries added stay as simulator libraries were
// compiled against them)
static_assert(sizeof(mwhip_ray_source) == 16 && sizeof(mwhip_box_plan) == 104 &&
              sizeof(mwhip_box_args) == 56);

namespace {

using madrona::MWCudaExecutor;
using madrona::MWHipContactQuery;
using madrona::py::Tensor;

static_assert(std::is_same_v<decltype(std::declval<MWCudaExecutor &>().makeContactQuery(
                                 std::declval<const mwhip_contacts_desc &>())),
                             MWHipContactQuery>);
static_assert(std::is_same_v<decltype(std::declval<MWCudaExecutor &>().setStepContacts(
                                 std::declval<const MWHipContactQuery *>(), true)), void>);
static_assert(std::is_same_v<decltype(std::declval<MWHipContactQuery &>().compute()), void>);
static_assert(std::is_same_v<decltype(std::declval<MWHipContactQuery &>().computeAsync()), void>);
static_assert(std::is_same_v<
    decltype(std::declval<const MWHipContactQuery &>().selectTensor()), Tensor>);
static_assert(std::is_same_v<
    decltype(std::declval<const MWHipContactQuery &>().statusTensor()), Tensor>);
static_assert(std::is_same_v<
    decltype(std::declval<const MWHipContactQuery &>().countsTensor()), Tensor>);
static_assert(std::is_same_v<
    decltype(std::declval<const MWHipContactQuery &>().pairsTensor()), Tensor>);
static_assert(std::is_same_v<
    decltype(std::declval<const MWHipContactQuery &>().numPointsTensor()), Tensor>);
static_assert(std::is_same_v<
    decltype(std::declval<const MWHipContactQuery &>().normalsTensor()), Tensor>);
static_assert(std::is_same_v<
    decltype(std::declval<const MWHipContactQuery &>().pointsTensor()), Tensor>);
static_assert(std::is_same_v<decltype(std::declval<const MWHipContactQuery &>().handleSource()),
                             mwhip_gather_source>);
static_assert(std::is_same_v<
    decltype(std::declval<const MWHipContactQuery &>().maxContacts()), uint64_t>);
static_assert(std::is_same_v<
    decltype(std::declval<const MWHipContactQuery &>().handle()), uint64_t>);

}

extern "C" {

#define CONTACTSCONF_API __attribute__((visibility("default")))
#define CONTACTSCONF_CAT2(a, b) a##b
#define CONTACTSCONF_CAT(a, b) CONTACTSCONF_CAT2(a, b)

// bit 0: default constructible, 1: not copy constructible, 2: not copy
// assignable, 3: move constructible, 4: move assignable
CONTACTSCONF_API uint32_t CONTACTSCONF_CAT(CONTACTSCONF_NAME, _traits)()
{
    return (std::is_default_constructible_v<MWHipContactQuery> ? 1u : 0u) |
        (!std::is_copy_constructible_v<MWHipContactQuery> ? 2u : 0u) |
        (!std::is_copy_assignable_v<MWHipContactQuery> ? 4u : 0u) |
        (std::is_move_constructible_v<MWHipContactQuery> ? 8u : 0u) |
        (std::is_move_assignable_v<MWHipContactQuery> ? 16u : 0u);
}

// the caps, flags and codes of the header, as this translation unit saw them
CONTACTSCONF_API uint32_t CONTACTSCONF_CAT(CONTACTSCONF_NAME, _caps)()
{
    return (uint32_t)MWHIP_MAX_STEP_CONTACTS << 16 | (uint32_t)MWHIP_CONTACTS_NUM_BUFS << 8 |
        (uint32_t)(MWHIP_CONTACTS_CURRENT_POSES | MWHIP_CONTACTS_PLAIN) << 4 |
        (uint32_t)(MWHIP_CONTACTS_OK - MWHIP_CONTACTS_UNSUPPORTED);
}

// every member once, on a caller's executor and a query that owns its select
// buffer; returns worlds x contacts (0: something was not as it should be)
CONTACTSCONF_API uint64_t CONTACTSCONF_CAT(CONTACTSCONF_NAME, _cycle)(
    MWCudaExecutor *exec, const mwhip_contacts_desc *desc)
{
    MWHipContactQuery first = exec->makeContactQuery(*desc);
    first.compute();
    first.computeAsync();
    exec->setStepContacts(&first, true);
    exec->setStepContacts(&first, false);
    MWHipContactQuery second(std::move(first));
    MWHipContactQuery third;
    third = std::move(second);
    const Tensor select = third.selectTensor();
    const Tensor status = third.statusTensor();
    const Tensor counts = third.countsTensor();
    const Tensor pairs = third.pairsTensor();
    const Tensor num_points = third.numPointsTensor();
    const Tensor normals = third.normalsTensor();
    const Tensor points = third.pointsTensor();
    const mwhip_gather_source source = third.handleSource();
    const int64_t worlds = status.dims()[0];
    if (third.handle() == 0 || select.numDims() != 1 || status.numDims() != 1 ||
            counts.numDims() != 1 || pairs.numDims() != 3 || num_points.numDims() != 2 ||
            normals.numDims() != 3 || points.numDims() != 3 || !status.isOnGPU() ||
            select.dims()[0] != worlds || counts.dims()[0] != worlds ||
            pairs.dims()[1] != (int64_t)third.maxContacts() || pairs.dims()[2] != 4 ||
            num_points.dims()[1] != (int64_t)third.maxContacts() || normals.dims()[2] != 3 ||
            points.dims()[2] != 16 || source.src != pairs.devicePtr() ||
            source.num_records != (uint64_t)worlds * third.maxContacts() * 2u ||
            source.record_bytes != 8u || source.handles_per_record != 1u) {
        return 0;
    }
    return (uint64_t)worlds * third.maxContacts();
}

}
